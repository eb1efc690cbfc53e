"""The storage leaf kernel computes the junctions (lcp + segment flags) of
its own entries, the segment ids are scanned after it and looked up where
they are consumed. Every state here is checked against the C oracle (root
and per-account storage roots), and every case first asserts from the
arrays alone that the boundary index or shared-nibble count it is about
really occurs."""
import numpy as np
import pytest

from oracle import bind, pyref
from tests.util import to_arrays

pytestmark = pytest.mark.gpu

CODE = pyref.KECCAK_EMPTY


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


def _akey(j):
    """Account key number j: ascending in j."""
    return (j + 1).to_bytes(2, "big") + bind.keccak256(b"lj-acct%d" % j)[2:]


def _skeys(tag, n):
    return [bind.keccak256(b"lj-slot-%s-%d" % (tag, t)) for t in range(n)]


def _state(counts):
    """One account per entry of counts, with that many slots (0 = an account
    without storage)."""
    accounts = {}
    for j, n in enumerate(counts):
        slots = {k: 1 + t + (j << 12)
                 for t, k in enumerate(_skeys(b"%d" % j, n))}
        accounts[_akey(j)] = (j, 1000 + j, CODE, slots)
    return to_arrays(accounts)


def _nibbles(key):
    k = np.asarray(key, np.uint8)
    return np.stack([k >> 4, k & 0xF], -1).reshape(-1)


def _lcp(a, b):
    d = np.nonzero(_nibbles(a) != _nibbles(b))[0]
    return 64 if len(d) == 0 else int(d[0])


def _junction(st, i):
    """lcp byte of rows i-1, i: -1 at a segment boundary or the array end."""
    if i <= 0 or i >= len(st):
        return -1
    if not np.array_equal(st[i - 1]["acct_key"], st[i]["acct_key"]):
        return -1
    return _lcp(st[i - 1]["slot_key"], st[i]["slot_key"])


def _check(eng, acct, st):
    want = bind.state_root(acct, st)
    eng.upload(acct, st)
    assert eng.root() == want
    assert np.array_equal(eng.storage_roots(len(acct)),
                          bind.storage_roots(acct, st))
    return want


# ---- boundary positions ---------------------------------------------------

@pytest.mark.parametrize("ns", [1, 2, 63, 64, 65, 255, 256, 257, 513])
def test_two_segment_boundary_positions(eng, ns):
    bounds = sorted({b for b in (1, 63, 64, 65, 255, 256, 257, ns - 1)
                     if 0 < b < ns})
    if ns == 1:
        acct, st = _state([1])
        assert len(st) == 1
        _check(eng, acct, st)
    for b in bounds:
        acct, st = _state([b, ns - b])
        assert len(st) == ns and _junction(st, b) == -1
        assert all(_junction(st, i) >= 0 for i in range(1, ns) if i != b)
        _check(eng, acct, st)


def test_300_single_slot_segments(eng):
    acct, st = _state([1] * 300)
    assert len(st) == 300
    assert all(_junction(st, i) == -1 for i in range(301))
    _check(eng, acct, st)


def test_single_slot_runs_across_wave_and_block_edges(eng):
    # entries 60..69 and 250..261 are single-slot segments; storage-less
    # accounts sit between accounts with storage
    counts = [60] + [1] * 4 + [0] + [1] * 6 + [180] + [0, 0] + [1] * 12 + [30]
    acct, st = _state(counts)
    assert len(st) == 60 + 10 + 180 + 12 + 30
    for lo, hi, edge in ((60, 70, 64), (250, 262, 256)):
        assert lo < edge < hi
        assert all(_junction(st, i) == -1 for i in range(lo, hi + 1))
    with_storage = {bytes(k) for k in st["acct_key"]}
    empty = [i for i, k in enumerate(acct["key"]) if bytes(k) not in with_storage]
    assert len(empty) == 3 and 0 < min(empty) and max(empty) < len(acct) - 1
    _check(eng, acct, st)
    roots = eng.storage_roots(len(acct))
    for i in empty:
        assert bytes(roots[i]) == pyref.EMPTY_ROOT_HASH


def test_accounts_without_storage_between(eng):
    counts = [3, 0, 70, 0, 0, 1, 0, 200, 0]
    acct, st = _state(counts)
    assert [int(np.sum(np.all(st["acct_key"] == k, axis=1)))
            for k in acct["key"]] == counts
    _check(eng, acct, st)


# ---- neighbours across the wave and block edge ----------------------------

def _pair_sharing(k, tag):
    """Two keys, ascending, sharing exactly k nibbles."""
    base = bytearray(bind.keccak256(b"lj-pair-%s-%d" % (tag, k)))
    base[0] = 0x80 | (base[0] & 0x0F)  # mid-range: random keys on both sides
    lo, hi = bytearray(base), bytearray(bind.keccak256(bytes(base)))
    hi[:k // 2] = base[:k // 2]
    if k & 1:
        lo[k >> 1] = (base[k >> 1] & 0xF0) | 0x4
        hi[k >> 1] = (base[k >> 1] & 0xF0) | 0xB
    else:
        lo[k >> 1] = 0x40 | (lo[k >> 1] & 0x0F)
        hi[k >> 1] = 0xB0 | (hi[k >> 1] & 0x0F)
    return bytes(lo), bytes(hi)


def _segment_with_pair(p, k):
    """Slot keys of one segment of p + 40 entries, sorted, whose entries
    p-1 and p share exactly k nibbles."""
    lo, hi = _pair_sharing(k, b"%d" % p)
    pool = _skeys(b"pool-%d-%d" % (p, k), 16 * (p + 40))
    below = [x for x in pool if x < lo][:p - 1]
    above = [x for x in pool if x > hi][:40 - 1]
    assert len(below) == p - 1 and len(above) == 39
    return sorted(below) + [lo, hi] + sorted(above)


@pytest.mark.parametrize("k", [0, 1, 12, 13, 14, 15, 16, 31, 32, 47, 48, 62, 63])
@pytest.mark.parametrize("p", [64, 256])
def test_pair_across_edge_shares_k_nibbles(eng, p, k):
    keys = _segment_with_pair(p, k)
    accounts = {
        _akey(0): (1, 1, CODE, {x: 7 + t for t, x in enumerate(keys)}),
        _akey(1): (2, 2, CODE, {x: 9 + t for t, x in enumerate(_skeys(b"t", 5))}),
    }
    acct, st = to_arrays(accounts)
    assert _junction(st, p) == k          # rows p-1 | p: wave / block edge
    assert _junction(st, p + 40) == -1    # then the second segment
    if k >= 12:  # the pair's own junction decides both leaves' depth
        assert _junction(st, p - 1) < k and _junction(st, p + 1) < k
    _check(eng, acct, st)


# ---- no read outside the array ---------------------------------------------

@pytest.mark.parametrize("n", [256, 300])
def test_trap_rows_around_a_borrowed_slice(eng, n):
    import torch
    acct, st = _state([n - 100, 100])
    assert len(st) == n
    big = np.zeros(n + 2, dtype=st.dtype)
    big[1:n + 1] = st
    # trap rows: same account as their neighbour, slot key sharing 20
    # nibbles with it, correctly ordered
    for trap, nb, byte in ((0, 1, 0x00), (n + 1, n, 0xFF)):
        big[trap] = big[nb]
        big["slot_key"][trap, 10:] = byte
        big["slot_key"][nb, 10] = 0x55
    st = big[1:n + 1].copy()
    assert _lcp(big[0]["slot_key"], big[1]["slot_key"]) == 20
    assert _lcp(big[n]["slot_key"], big[n + 1]["slot_key"]) == 20
    assert bytes(big[0]["slot_key"]) < bytes(big[1]["slot_key"])
    assert bytes(big[n]["slot_key"]) < bytes(big[n + 1]["slot_key"])
    for i in range(n + 2):
        assert i in (0, n + 1) or np.array_equal(big[i], st[i - 1])
    # in-array neighbours share fewer nibbles: a read of a trap row would
    # deepen the end leaf and change the root
    assert 0 <= _junction(st, 1) < 20 and 0 <= _junction(st, n - 1) < 20
    want = bind.state_root(acct, st)
    # the trap rows are valid entries: with them in, the root differs
    assert bind.state_root(acct, big) != want
    acct_t = torch.from_numpy(acct.view(np.uint8).reshape(-1, 104).copy()).cuda()
    big_t = torch.from_numpy(big.view(np.uint8).reshape(-1, 96).copy()).cuda()
    eng.set_device_tensors(acct_t, big_t[1:n + 1])
    assert eng.root() == want
    assert np.array_equal(eng.storage_roots(len(acct)),
                          bind.storage_roots(acct, st))
    eng.upload(acct, st)  # drop the borrow
    eng.release_borrowed()


# ---- input contract ---------------------------------------------------------

def _contract_cases():
    acct, st = _state([130, 70])
    ns = len(st)
    cases = []
    for a, b in ((0, 1), (63, 64), (ns - 2, ns - 1)):
        bad = st.copy()
        bad["slot_key"][b] = bad["slot_key"][a]
        cases.append(("dup-%d" % a, bad, "storage-not-sorted-or-duplicate",
                      lambda s, a=a, b=b: _junction(s, b) == 64))
    bad = st.copy()
    bad[[10, 11]] = bad[[11, 10]]
    cases.append(("descending-slot", bad, "storage-not-sorted-or-duplicate",
                  lambda s: bytes(s[10]["slot_key"]) > bytes(s[11]["slot_key"])
                  and np.array_equal(s[10]["acct_key"], s[11]["acct_key"])))
    bad = np.concatenate([st[130:], st[:130]])
    cases.append(("descending-acct", bad, "storage-not-sorted-or-duplicate",
                  lambda s: bytes(s[69]["acct_key"]) > bytes(s[70]["acct_key"])))
    bad = st.copy()
    bad["acct_key"][130:] = np.frombuffer(_akey(5), np.uint8)
    cases.append(("orphan", bad, "storage-for-unknown-account",
                  lambda s: bytes(s[130]["acct_key"]) not in
                  {bytes(k) for k in acct["key"]}
                  and bytes(s[129]["acct_key"]) < bytes(s[130]["acct_key"])))
    bad = st.copy()
    bad["value"][77] = 0
    cases.append(("zero-value", bad, "zero-storage-value",
                  lambda s: not s[77]["value"].any()))
    return acct, st, cases


@pytest.mark.parametrize("idx", range(7))
def test_input_contract(eng, idx):
    acct, st, cases = _contract_cases()
    assert len(cases) == 7
    name, bad, msg, occurs = cases[idx]
    assert occurs(bad), name
    eng.upload(acct, bad)
    with pytest.raises(RuntimeError, match=msg):
        eng.root()
    _check(eng, acct, st)


# ---- consumers of the looked-up segment id ---------------------------------

@pytest.fixture(scope="module")
def three():
    accounts = {}
    for j, n in enumerate((290, 310, 300)):
        accounts[_akey(j)] = (j, 5 + j, CODE, {
            k: 3 + t for t, k in enumerate(_skeys(b"three-%d" % j, n))})
    acct, st = to_arrays(accounts)
    starts = [i for i in range(len(st)) if _junction(st, i) == -1]
    assert starts == [0, 290, 600] and all(s % 256 for s in starts[1:])
    return accounts, acct, st


@pytest.mark.parametrize("cls_min", [None, "1"])
def test_three_segments_roots(eng, three, monkeypatch, cls_min):
    # "1" sends the root branches through the class partition and the fused
    # one-block kernel as well
    if cls_min:
        monkeypatch.setenv("SRE_CLS_MIN", cls_min)
    _, acct, st = three
    _check(eng, acct, st)


def test_three_segments_update_rows(eng, three):
    _, acct, st = three
    want_root, want_rows = bind.state_root_with_updates(acct, st)
    # stored branches below the root whose interval does not start at the
    # segment start, in the second and third segment
    for j in (1, 2):
        key = acct[j]["key"]
        first_nib = int(st[[0, 290, 600][j]]["slot_key"][0]) >> 4
        rows = [r for r in want_rows if r["kind"] == 1 and r["path_len"] >= 1
                and np.array_equal(r["acct_key"], key)
                and int(r["path"][0]) >> 4 != first_nib]
        assert rows, j
    eng.upload(acct, st)
    got_root, got_rows = eng.root_with_updates()
    assert got_root == want_root
    assert len(got_rows) == len(want_rows), (len(got_rows), len(want_rows))
    ga = got_rows.view(np.uint8).reshape(len(got_rows), -1)
    wa = want_rows.view(np.uint8).reshape(len(want_rows), -1)
    if not np.array_equal(ga, wa):
        for i in range(len(got_rows)):
            if not np.array_equal(ga[i], wa[i]):
                raise AssertionError(
                    f"row {i}: engine={got_rows[i]} oracle={want_rows[i]}")


def test_three_segments_storage_proofs(eng, three):
    accounts, acct, st = three
    pairs = [(bytes(st[i]["acct_key"]), bytes(st[i]["slot_key"]))
             for i in (300, 599, 600, 777)]
    assert [a for a, _ in pairs] == [_akey(1), _akey(1), _akey(2), _akey(2)]
    eng.upload(acct, st)
    roots, proofs = eng.storage_proof([a for a, _ in pairs],
                                      [s for _, s in pairs])
    for (a, s), root, nodes in zip(pairs, roots, proofs):
        with pyref.accelerated(bind.keccak256):
            wroot, wnodes = pyref.storage_proof({a: accounts[a]}, a, s)
        assert root == wroot and nodes == wnodes and nodes, a.hex()


def test_three_segments_subtree_roots(eng, three):
    _, acct, st = three
    want = bind.state_root(acct, st)
    eng.upload(acct, st)
    refs, lens, roots, counts = eng.subtree_roots()
    o_refs, o_lens, o_roots, o_counts = bind.subtree_roots(acct, st)
    assert np.array_equal(refs, o_refs) and np.array_equal(lens, o_lens)
    assert np.array_equal(roots, o_roots) and np.array_equal(counts, o_counts)
    assert eng.finish_top(refs, lens, roots, counts) == want
