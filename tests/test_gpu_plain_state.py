"""Plain-state upload on the GPU (include/sre.h sre_upload_plain_state,
sre_set_plain_state_device, sre_download_*, sre_get_hash_sort_counters)
against tests/plain_model.py: the resident rows byte for byte, and every
counter.

Boundaries of the implementation (reth_amd/csrc/radix.h and hs_sort_pairs in
sre.hip), each covered with -1 / 0 / +1 rows:

  64      one wave round (HS_WAVE): the peer-mask ballots
  512     one wave's span of a tile (HS_WAVE_SPAN): the cross-wave counts
  2048    one tile (HS_TILE): more than one block, the [digit][tile] scan
  16384   8 tiles = 2048 histogram cells per scan block x 256 digits: from
          16385 rows on the scan of the matrix takes its second level
  256 / 65536 accounts: the storage key's rank grows by one byte, i.e. one
          more executed pass (257 and 70 001 accounts)

The scan's third level starts at 2048 scan blocks = 33.5M rows, out of a
quick test's reach; the second level runs the same code recursively.

Per-account slot counts 1, 63, 64, 65, 255, 256, 257 sit in one state so
that the groups of one account cross wave and block widths of the one-lane-
per-row key and gather kernels.
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import bind, pyref
from reth_amd import gen, plain
from reth_amd.engine import DELTA_DTYPE
from tests import plain_model as pm
from tests.test_gpu_incremental import _arrays_of, _dict_of, _mk_delta
from tests.test_gpu_proof import _dict_of as _tuple_dict_of

pytestmark = pytest.mark.gpu

GATE = "SRE_HS_KEY_BITS"
SLOT_MIX = [1, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


@pytest.fixture()
def key_bits(request):
    """Sets the sort-key gate (read by the engine on every call) and removes
    it afterwards."""
    os.environ[GATE] = str(request.param)
    yield request.param
    os.environ.pop(GATE, None)


_MODELS = {}


def _state(na, slots_tag):
    """(plain accounts, plain storage, Model), computed once per shape."""
    key = (na, slots_tag)
    if key not in _MODELS:
        if slots_tag == "mix":
            counts = np.array((SLOT_MIX * (na // len(SLOT_MIX) + 1))[:na])
        elif slots_tag == "sparse":  # one slot for every third account
            counts = (np.arange(na) % 3 == 1).astype(np.int64)
        elif slots_tag == "sparse+mix":  # ... and every 59th takes SLOT_MIX
            counts = (np.arange(na) % 3 == 1).astype(np.int64)
            heavy = np.arange(0, na, 59)
            counts[heavy] = (SLOT_MIX * len(heavy))[:len(heavy)]
        else:
            counts = slots_tag
        a, s = plain.gen_plain_numpy(na, counts)
        _MODELS[key] = (a, s, pm.Model(a, s))
    return _MODELS[key]


def _same(eng, m, key_bits=None):
    acct, st = eng.download()
    assert eng.resident_counts() == (len(m.acct), len(m.st))
    assert acct.tobytes() == m.acct.tobytes()
    assert st.tobytes() == m.st.tobytes()
    got, want = eng.hash_sort_counters(), m.counters(key_bits)
    print("counters", got, "model", want)
    assert got == want


# ---- genesis ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["mainnet", "sepolia", "holesky"])
def test_genesis_from_shuffled_plain_rows(eng, name):
    acct, st, root = pm.genesis_plain(name, seed=3)
    eng.upload_plain(acct, st)
    assert eng.root() == root


# ---- row for row -----------------------------------------------------------

ACCOUNT_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048,
                  2049, 4095, 4096, 4097, 16383, 16384, 16385, 70001]


@pytest.mark.parametrize("na", ACCOUNT_COUNTS)
def test_rows_and_counters_by_account_count(eng, na):
    a, s, m = _state(na, "sparse")
    eng.upload_plain(*pm.shuffled(a, s, na))
    _same(eng, m)
    if na in (0, 1, 2049, 70001):
        assert eng.root() == bind.state_root(m.acct, m.st)


def test_no_storage_and_one_storage_row(eng):
    a, s, m = _state(300, 0)
    assert len(s) == 0
    eng.upload_plain(*pm.shuffled(a, s, 1))
    _same(eng, m)
    a, s = plain.gen_plain_numpy(3, np.array([0, 1, 0]))
    m = pm.Model(a, s)
    assert len(s) == 1
    eng.upload_plain(a, s)
    _same(eng, m)
    assert eng.root() == bind.state_root(m.acct, m.st)


@pytest.mark.parametrize("order", ["sorted", "reversed", "shuffled", "grouped"])
def test_slot_counts_across_wave_and_block_widths(eng, order):
    a, s, m = _state(70, "mix")  # 10 of each count: 9610 rows, 5 tiles
    if order == "sorted":
        a2, s2 = a[m.order], s[m.sorder]
    elif order == "reversed":
        a2, s2 = a[m.order][::-1].copy(), s[m.sorder][::-1].copy()
    elif order == "shuffled":
        a2, s2 = pm.shuffled(a, s, 5)
    else:  # storage grouped by address as PlainStorageState is, accounts not
        a2, s2 = pm.shuffled(a, s[:0], 6)[0], s
    eng.upload_plain(a2, s2)
    _same(eng, m)
    assert eng.root() == bind.state_root(m.acct, m.st)


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_200k_storage_rows(eng, order):
    a, s, m = _state(3125, 64)
    assert len(s) == 200_000
    a2, s2 = pm.shuffled(a, s, 9)
    eng.upload_plain(a2, s if order == "grouped" else s2)
    _same(eng, m)
    assert eng.root() == bind.state_root(m.acct, m.st)


def test_device_tensors_are_read_only_inputs(eng):
    import torch
    a, s, m = _state(4097, "sparse+mix")
    a2, s2 = pm.shuffled(a, s, 2)
    ta, ts = plain.np_plain_to_tensors(a2, s2, device="cuda")
    ca, cs = ta.clone(), ts.clone()
    eng.set_plain_device_tensors(ta, ts)
    torch.cuda.synchronize()
    assert torch.equal(ta, ca) and torch.equal(ts, cs)
    del ta, ts  # the engine kept no reference
    _same(eng, m)
    assert eng.root() == bind.state_root(m.acct, m.st)


# ---- ties carry the sort ---------------------------------------------------

@pytest.mark.parametrize("key_bits", [0, 4, 9], indirect=True)
def test_ties_carry_the_sort(eng, key_bits):
    # K = 0 leaves one run per account sort and one per account: one thread
    # orders each, so that case stays at 512 accounts
    a, s, m = _state(512 if key_bits == 0 else 4097, "sparse+mix")
    want = m.counters(key_bits)
    # pigeonhole: more than 2^K keys per state (accounts) or account (slots)
    assert want["tie_rows"] > 0 and want["tie_runs"] > 0
    assert want["passes"] < m.counters()["passes"]
    eng.upload_plain(*pm.shuffled(a, s, key_bits))
    _same(eng, m, key_bits)
    assert eng.root() == bind.state_root(m.acct, m.st)


# ---- pass skipping ---------------------------------------------------------

@pytest.mark.parametrize("na,slots,st_passes", [(1, 300, 4), (255, 2, 5),
                                                (257, 2, 6), (70001, 1, 7)])
def test_storage_passes_follow_the_rank_width(eng, na, slots, st_passes):
    a, s, m = _state(na, slots)
    (_, _), (st_ran, st_skipped) = m.passes()
    assert (st_ran, st_skipped) == (st_passes, 8 - st_passes)
    eng.upload_plain(*pm.shuffled(a, s, 4))
    _same(eng, m)


# ---- rejections ------------------------------------------------------------

@pytest.fixture(scope="module")
def resident():
    """The state that is resident before every rejected call."""
    acct, st = gen.gen_state_numpy(64, 2, bind.keccak256_batch)
    return acct, st, bind.state_root(acct, st)


def _orphans(m):
    """Addresses outside the state hashing below the first account key,
    above the last, and between two."""
    cand, _ = plain.gen_plain_numpy(4000, 0, first=1_000_000)
    h = bind.keccak256_batch(cand["address"].reshape(-1, 20))
    keys = [bytes(k) for k in m.acct["key"]]
    lo, hi = keys[0], keys[-1]
    out = {}
    for addr, hk in zip(cand["address"], h):
        hk = bytes(hk)
        if hk < lo:
            out.setdefault("below", addr)
        elif hk > hi:
            out.setdefault("above", addr)
        elif hk not in keys:  # lo < hk < hi: between two account keys
            out.setdefault("between", addr)
    assert set(out) == {"below", "above", "between"}
    return out


def _bad_inputs():
    a, s, m = _state(64, 3)
    out = {}
    d = np.concatenate([a[:6], a[5:6], a[6:]])
    d[6]["nonce"] += 1
    out["dup-address-adjacent"] = (d, s, "duplicate-address")
    big, bs, _ = _state(5000, "sparse")
    d = np.concatenate([big[:4500], big[10:11], big[4500:]])  # tiles 0 and 2
    out["dup-address-far"] = (d, bs, "duplicate-address")
    d = np.concatenate([s, s[100:101]])
    d[-1]["value"][0] = 0x11  # another, still nonzero, value
    out["dup-storage-slot"] = (a, d, "duplicate-storage-slot")
    for where, addr in _orphans(m).items():
        d = s.copy()
        d[17]["address"] = addr
        out["orphan-" + where] = (a, d, "storage-for-unknown-account")
    d = s.copy()
    d[40]["value"] = 0
    out["zero-value"] = (a, d, "zero-storage-value")
    return out


BAD = ["dup-address-adjacent", "dup-address-far", "dup-storage-slot",
       "orphan-below", "orphan-above", "orphan-between", "zero-value"]


def _rejected(eng, resident, accounts, storage, token):
    acct, st, root = resident
    eng.upload(acct, st)
    assert eng.root_retaining() == root
    before = eng.hash_sort_counters()
    with pytest.raises(RuntimeError) as ei:
        eng.upload_plain(accounts, storage)
    msg = str(ei.value)
    assert token in msg and "internal" not in msg, msg
    assert eng.root() == root
    got_a, got_s = eng.download()
    assert got_a.tobytes() == acct.tobytes() and got_s.tobytes() == st.tobytes()
    assert eng.hash_sort_counters() == before
    # retention is as before the call: an incremental step needs no re-arm
    assert eng.incremental_root(np.zeros(0, DELTA_DTYPE)) == root


@pytest.mark.parametrize("case", BAD)
def test_rejected_plain_upload_changes_nothing(eng, resident, case):
    accounts, storage, token = _bad_inputs()[case]
    _rejected(eng, resident, accounts, storage, token)


@pytest.mark.parametrize("key_bits", [4], indirect=True)
def test_duplicate_inside_a_long_tie_run(eng, resident, key_bits):
    a, s, m = _state(600, 0)
    assert m.counters(key_bits)["tie_runs"] <= 16  # runs of ~40 rows
    d = np.concatenate([a, a[123:124]])
    _rejected(eng, resident, d, s, "duplicate-address")
    a, s, m = _state(1, 300)
    d = np.concatenate([s[:7], s[250:251], s[7:]])
    _rejected(eng, resident, a, d, "duplicate-storage-slot")


# ---- downstream ------------------------------------------------------------

def test_downstream_calls_after_plain_upload(eng):
    a, s, m = _state(800, 3)
    eng.upload_plain(*pm.shuffled(a, s, 8))
    assert (eng.storage_roots(len(m.acct)) ==
            bind.storage_roots(m.acct, m.st)).all()
    tuples = _tuple_dict_of(m.acct, m.st)
    keys = sorted(tuples)
    target = keys[777]
    assert eng.account_proof([target]) == [pyref.account_proof(tuples, target)]

    accounts = _dict_of(m.acct, m.st)
    assert eng.root_retaining() == bind.state_root(m.acct, m.st)
    rows, strows = [], []
    for k in keys[100:105]:
        v = accounts[k]
        v[1] += 7
        rows.append((k, v[0], v[1], v[2], 0))
    sk = bind.keccak256(b"fresh-slot")
    accounts[keys[300]][3][sk] = 99
    strows.append((keys[300], sk, 99))
    d, sd = _mk_delta(rows, strows)
    assert eng.incremental_root(d, sd) == bind.state_root(*_arrays_of(accounts))


# ---- download alone --------------------------------------------------------

def test_download_after_upload_and_apply_delta(eng):
    acct, st = gen.gen_state_numpy(500, 3, bind.keccak256_batch)
    eng.upload(acct, st)
    got_a, got_s = eng.download()
    assert got_a.tobytes() == acct.tobytes() and got_s.tobytes() == st.tobytes()

    accounts = _dict_of(acct, st)
    keys = sorted(accounts)
    ke = bind.keccak256(b"")
    rows = [(keys[3], 0, 0, ke, 1)]  # destroyed: storage goes too
    del accounts[keys[3]]
    nk = bind.keccak256(b"download-new")
    accounts[nk] = [1, 5, ke, {}]
    rows.append((nk, 1, 5, ke, 0))
    dead = sorted(accounts[keys[9]][3])[0]
    del accounts[keys[9]][3][dead]
    strows = [(keys[9], dead, 0)]
    eng.apply_delta(*_mk_delta(rows, strows))
    want_a, want_s = _arrays_of(accounts)
    got_a, got_s = eng.download()
    assert got_a.tobytes() == want_a.tobytes()
    assert got_s.tobytes() == want_s.tobytes()

    # a wrong n is an argument error, and nothing is written
    na, ns = eng.resident_counts()
    buf = np.zeros(na + 1, dtype=got_a.dtype)
    for fn, n in ((eng._lib.sre_download_accounts, na + 1),
                  (eng._lib.sre_download_accounts, na - 1),
                  (eng._lib.sre_download_storage, ns + 1)):
        rc = fn(ctypes.c_void_p(eng._ctx), buf.ctypes.data_as(ctypes.c_void_p),
                ctypes.c_uint64(n))
        assert rc != 0
        msg = eng._lib.sre_last_error(ctypes.c_void_p(eng._ctx)).decode()
        assert "rows are resident" in msg and "internal" not in msg
    assert not buf.view(np.uint8).any()
