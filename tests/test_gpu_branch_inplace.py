"""Branch kernels place their own nodes (branch_tail stores to recs[s] /
depths[s]; roots and error groups store nothing).

The shapes are the smallest at which that store can go wrong:

- one level with exactly 255, 256, 257, 511, 512 and 513 groups, 2-3-child
  and 4+-child branches mixed: under SRE_CLS_MIN=1 SRE_BR_CHUNK=256 that is
  the chunk edge, the class-0 slice split over both streams and the split
  assemble/hash pipeline on one level, each kernel placing its own nodes;
- a non-root branch whose interval starts at slot 0 and one at slot n-2, the
  last place a 48-byte record fits;
- tries whose root branch sits at depth > 0 (an extension above it, no
  record stored, the slot's depth byte left stale) between large tries, in
  storage tries and in the account trie; also through subtree_roots +
  finish_top;
- one state holding all of the above through root_with_updates, an account
  and a storage multiproof, and root_retaining + incremental_root;
- one chained sequence of differently sized calls on one engine, so pooled
  buffers change hands between the calls.

Every shape property (group counts, slot positions, root depths) is asserted
in Python from the sorted keys before any root is trusted. Every case
compares the root and the per-account storage roots with the C oracle and
requires stats()["branch_count"] and ["levels"] to equal _branch_levels of
the keys, under the default gates and under SRE_CLS_MIN=1 SRE_BR_CHUNK=256.
"""
import functools
import os

import numpy as np
import pytest

from oracle import bind, pyref
from tests.test_gpu_incremental import _mk_delta
from tests.test_gpu_inplace_levels import _check_root, _levels_of, _members
from tests.test_gpu_pipeline_gates import _branch_levels
from tests.test_gpu_proof import _replay
from tests.util import to_arrays

pytestmark = pytest.mark.gpu

KE = pyref.KECCAK_EMPTY
CONFIGS = {
    "base": {},
    "cls+chunk": {"SRE_CLS_MIN": "1", "SRE_BR_CHUNK": "256"},
}
CHUNK = 256
GROUP_COUNTS = (255, 256, 257, 511, 512, 513)
GROUP_DEPTH = 3
# children per group, cycled: class 0 (<= 3 children, the fused kernel) and
# classes 1-3 (the split pipeline), a full 16-child branch among them
CHILDREN = (2, 3, 4, 2, 3, 7, 2, 16, 3, 5)


@pytest.fixture(scope="module", params=list(CONFIGS))
def eng(request):
    env = CONFIGS[request.param]
    for v in env:
        assert v not in os.environ, v
    os.environ.update(env)  # the gates are read per call
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()
    for v in env:
        os.environ.pop(v, None)


# --------------------------------------------------------------------------
# states
# --------------------------------------------------------------------------

def _key(prefix, tag):
    """32-byte key: the given leading nibbles, the rest from keccak(tag)."""
    head = "".join("%x" % n for n in prefix)
    return bytes.fromhex(head + bind.keccak256(tag).hex()[len(head):])


def _akey(i):
    """Account keys that sort by i."""
    return (i + 1).to_bytes(2, "big") + bind.keccak256(b"bi-acct%d" % i)[2:]


def group_keys(n_groups, tag):
    """n_groups branch nodes at depth GROUP_DEPTH, group g with
    CHILDREN[g % 10] leaf children; no branch below that depth."""
    keys = []
    for g in range(n_groups):
        for k in range(CHILDREN[g % len(CHILDREN)]):
            child = (5 * k + g) % 16  # distinct for k < 16
            keys.append(_key((g >> 8, (g >> 4) & 15, g & 15, child),
                             tag + b"%d/%d" % (g, k)))
    return keys


def _rand_keys(n, tag):
    return [bind.keccak256(tag + b"%d" % j) for j in range(n)]


def _slots(keys, base=1):
    return {k: base + j for j, k in enumerate(keys)}


def _acct(i, keys):
    return {_akey(i): (1, 1000 + i, KE, _slots(keys, 1 + (i << 12)))}


def _accounts(keys):
    return {k: (i % 7, 10 ** 12 + i, KE, {}) for i, k in enumerate(keys)}


def groups_storage(n_groups, first=0):
    acc = {}
    acc.update(_acct(first, _rand_keys(3, b"bi-g-small")))
    acc.update(_acct(first + 1, group_keys(n_groups, b"bi-gs%d/" % n_groups)))
    acc.update(_acct(first + 2, _rand_keys(2, b"bi-g-two")))
    return acc


# two keys sharing five nibbles below everything else, two above
LOW_PAIR = [_key((0, 0, 0, 0, 0, 1), b"bi-lo1"), _key((0, 0, 0, 0, 0, 2), b"bi-lo2")]
HIGH_PAIR = [_key((15, 15, 15, 15, 15, 1), b"bi-hi1"),
             _key((15, 15, 15, 15, 15, 14), b"bi-hi2")]
EDGE_DEPTH = 5


def _between(n, tag):
    """Random keys strictly between the pairs' top nibbles."""
    return [_key((1 + j % 14,), tag + b"%d" % j) for j in range(n)]


def edge_storage(first=0):
    acc = {}
    acc.update(_acct(first, LOW_PAIR + _between(3, b"bi-e0-")))
    acc.update(_acct(first + 1, _rand_keys(40, b"bi-e1-")))
    acc.update(_acct(first + 2, _between(2, b"bi-e2-") + HIGH_PAIR))
    return acc


def edge_accounts():
    return _accounts(LOW_PAIR + _between(40, b"bi-ea-") + HIGH_PAIR)


DEEP3 = [_key((10, 11, 12, 1 + 3 * j), b"bi-d3-%d" % j) for j in range(5)]
DEEP7 = [_key((4, 4, 4, 4, 4, 4, 4, 2 + 9 * j), b"bi-d7-%d" % j)
         for j in range(2)]


def deep_storage(first=0):
    """Storage tries rooted at depth 3 and 7 between large ones."""
    acc = {}
    acc.update(_acct(first, _rand_keys(300, b"bi-big0-")))
    acc.update(_acct(first + 1, DEEP3))
    acc.update(_acct(first + 2, _rand_keys(300, b"bi-big1-")))
    acc.update(_acct(first + 3, DEEP7))
    acc.update(_acct(first + 4, _rand_keys(257, b"bi-big2-")))
    return acc


def deep_accounts():
    """Account trie rooted at depth 2; two accounts carry storage."""
    keys = [_key((5, 5), b"bi-da-%d" % j) for j in range(300)]
    acc = _accounts(keys)
    for i, k in enumerate(sorted(keys)[100:102]):
        acc[k] = (1, 77 + i, KE, _slots(DEEP3 if i else _rand_keys(20, b"bi-das")))
    return acc


def combo():
    acc = groups_storage(257, first=0)
    acc.update(edge_storage(first=10))
    acc.update(deep_storage(first=20))
    return acc


STATES = {}
for _n in GROUP_COUNTS:
    STATES["gst%d" % _n] = functools.partial(groups_storage, _n)
    STATES["gac%d" % _n] = functools.partial(
        lambda n: _accounts(group_keys(n, b"bi-ga%d/" % n)), _n)
STATES.update({
    "edge_storage": edge_storage,
    "edge_accounts": edge_accounts,
    "deep_storage": deep_storage,
    "deep_accounts": deep_accounts,
    "combo": combo,
})


class Ref:
    def __init__(self, name):
        self.accounts = STATES[name]()
        self.acct, self.st = to_arrays(self.accounts)
        self.root = bind.state_root(self.acct, self.st)
        self.sroots = bind.storage_roots(self.acct, self.st)
        self.subtree = bind.subtree_roots(self.acct, self.st)
        # tries as (first entry, sorted hex keys), in entry order
        self.st_tries = []
        n = 0
        for _, (_, _, _, slots) in sorted(self.accounts.items()):
            if slots:
                self.st_tries.append((n, sorted(k.hex() for k in slots)))
                n += len(slots)
        assert n == len(self.st)
        self.ac_tries = [(0, sorted(k.hex() for k in self.accounts))]
        self.lv_storage = _branch_levels(k for _, k in self.st_tries)
        self.lv_account = _branch_levels(k for _, k in self.ac_tries)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return Ref(name)


# --------------------------------------------------------------------------
# the shape properties, from the sorted keys alone
# --------------------------------------------------------------------------

@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_group_level_shapes(n_groups):
    for name, lv in (("gst%d" % n_groups, ref_of("gst%d" % n_groups).lv_storage),
                     ("gac%d" % n_groups, ref_of("gac%d" % n_groups).lv_account)):
        assert max(lv) == GROUP_DEPTH, name
        total, small = lv[GROUP_DEPTH]
        assert total == n_groups, name
        # both the fused class and the split classes on the level
        assert small == sum(CHILDREN[g % 10] <= 3 for g in range(n_groups)), name
        assert 0 < small < total, name
    # chunk edge: one group short of, exactly on and one past 1 and 2 chunks
    assert sorted({n - CHUNK * (n // CHUNK) for n in GROUP_COUNTS}) == \
        [0, 1, CHUNK - 1]
    assert 16 in CHILDREN and 2 in CHILDREN and 3 in CHILDREN


def _starts(tries, depth):
    return [m[0] for m in _members(tries).get(depth, [])]


def test_edge_slot_shapes():
    for name, tries, n in (
            ("edge_storage", ref_of("edge_storage").st_tries,
             len(ref_of("edge_storage").st)),
            ("edge_accounts", ref_of("edge_accounts").ac_tries,
             len(ref_of("edge_accounts").acct))):
        starts = _starts(tries, EDGE_DEPTH)
        assert starts == [0, n - 2], (name, starts, n)
        # neither is a root: its trie has a branch at depth 0 above it
        roots = _starts(tries, 0)
        assert 0 in roots, name
        first_of_last_trie = tries[-1][0]
        assert first_of_last_trie in roots and first_of_last_trie < n - 2, name


def test_deep_root_shapes():
    r = ref_of("deep_storage")
    depths = [min(_branch_levels([keys])) for _, keys in r.st_tries]
    sizes = [len(keys) for _, keys in r.st_tries]
    assert depths == [0, 3, 0, 7, 0], depths
    assert sizes == [300, 5, 300, 2, 257], sizes
    r = ref_of("deep_accounts")
    assert min(r.lv_account) == 2 and len(r.acct) == 300
    assert sorted(min(_branch_levels([k])) for _, k in r.st_tries) == [0, 3]
    # the combined state keeps every property
    r = ref_of("combo")
    n = len(r.st)
    assert r.lv_storage[GROUP_DEPTH][0] >= 257
    assert {min(_branch_levels([k])) for _, k in r.st_tries} == {0, 3, 7}
    offs = [off for off, _ in r.st_tries]
    starts = _starts(r.st_tries, EDGE_DEPTH)
    assert any(s in offs for s in starts), starts      # the low pair
    assert any(s not in offs for s in starts), starts  # the high pair
    assert n == sum(len(k) for _, k in r.st_tries)


# --------------------------------------------------------------------------
# roots and counters
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(STATES))
def test_roots(eng, name):
    r = ref_of(name)
    eng.upload(r.acct, r.st)
    _check_root(eng, r.acct, r.st, r.root, r.sroots, r.lv_storage,
                r.lv_account, name)


@pytest.mark.parametrize("name", ["deep_storage", "deep_accounts", "combo",
                                  "gst513", "gac257"])
def test_subtree_roots_and_finish_top(eng, name):
    r = ref_of(name)
    eng.upload(r.acct, r.st)
    refs, lens, roots, counts = eng.subtree_roots()
    assert np.array_equal(lens, r.subtree[1]), name
    assert np.array_equal(refs, r.subtree[0]), name
    assert np.array_equal(roots, r.subtree[2]), name
    assert eng.finish_top(refs, lens, roots, counts) == r.root, name


# --------------------------------------------------------------------------
# the other surfaces that share branch_tail, on the combined state
# --------------------------------------------------------------------------

def test_updates(eng):
    r = ref_of("combo")
    want_root, want_rows = bind.state_root_with_updates(r.acct, r.st)
    assert want_root == r.root
    eng.upload(r.acct, r.st)
    root, rows = eng.root_with_updates()
    assert root == r.root
    assert len(rows) == len(want_rows) and len(rows) > 0
    assert rows.tobytes() == want_rows.tobytes(), "update rows"


def test_account_multiproof(eng):
    r = ref_of("combo")
    akeys = [bytes(k) for k in r.acct["key"]]
    targets = [akeys[0], akeys[len(akeys) // 2], akeys[-1],
               bind.keccak256(b"bi-absent")]
    items = sorted(
        (pyref.nibbles_of(k), pyref.account_value(
            int(a["nonce"]), int.from_bytes(bytes(a["balance"]), "big"),
            bytes(s), bytes(a["code_hash"])))
        for k, a, s in zip(akeys, r.acct, r.sroots))
    eng.upload(r.acct, r.st)
    proofs = eng.account_proof(targets)
    with pyref.accelerated(bind.keccak256):
        for t, nodes in zip(targets, proofs):
            want = []
            pyref._collect_proof(items, 0, pyref.nibbles_of(t), True, want)
            assert nodes == want, f"account proof {t.hex()}"
            assert (_replay(nodes, t, r.root) is not None) == (t in akeys)


def test_storage_multiproof(eng):
    r = ref_of("combo")
    grp, deep3, last = _akey(1), _akey(21), _akey(12)
    gk = sorted(r.accounts[grp][3])
    pairs = [(grp, gk[0]), (grp, gk[len(gk) // 2]), (grp, gk[-1]),
             (deep3, DEEP3[2]), (deep3, bind.keccak256(b"bi-absent-slot")),
             (last, HIGH_PAIR[0]), (last, HIGH_PAIR[1]),
             (_akey(10), LOW_PAIR[0])]
    for a, _ in pairs:
        assert r.accounts[a][3], a.hex()
    eng.upload(r.acct, r.st)
    roots, proofs = eng.storage_proof([a for a, _ in pairs],
                                      [s for _, s in pairs])
    for (a, s), root, nodes in zip(pairs, roots, proofs):
        with pyref.accelerated(bind.keccak256):
            wroot, wnodes = pyref.storage_proof(
                {a: (0, 0, b"", r.accounts[a][3])}, a, s)
        assert root == wroot, f"storage root {a.hex()}"
        assert nodes == wnodes, f"storage proof {a.hex()}/{s.hex()}"
        here = s in r.accounts[a][3]
        assert nodes or not here
        if nodes:
            assert (_replay(nodes, s, root) is not None) == here, s.hex()


def test_retaining_and_incremental(eng):
    r = ref_of("combo")
    acc = {k: (n, b, ch, dict(sl)) for k, (n, b, ch, sl) in r.accounts.items()}
    eng.upload(r.acct, r.st)
    assert eng.root_retaining() == r.root
    grp, deep3 = _akey(1), _akey(21)
    new = bind.keccak256(b"bi-new-acct")
    rows = [(deep3, 9, 10 ** 15, KE, 0), (new, 1, 5, KE, 0)]
    strows = [(grp, bind.keccak256(b"bi-new-slot"), 77),
              (grp, sorted(acc[grp][3])[3], 78)]
    for k, n, b, ch, _ in rows:
        acc[k] = (n, b, ch, acc.get(k, (0, 0, KE, {}))[3])
    for a, s, v in strows:
        acc[a][3][s] = v
    d, s = _mk_delta(rows, strows)
    acct2, st2 = to_arrays(acc)
    assert eng.incremental_root(d, s) == bind.state_root(acct2, st2)
    lvs, lva = _levels_of(acct2, st2)
    _check_root(eng, acct2, st2, bind.state_root(acct2, st2),
                bind.storage_roots(acct2, st2), lvs, lva, "root after delta")


def test_chained_calls_of_different_sizes(eng):
    """The size classes the per-level node buffer used to take from the
    pool now go to other buffers: big, small, big again on one engine."""
    for step, name in enumerate(["gst513", "edge_accounts", "combo", "gac255",
                                 "deep_storage", "gst256", "deep_accounts",
                                 "gac513", "edge_storage", "combo"]):
        r = ref_of(name)
        eng.upload(r.acct, r.st)
        _check_root(eng, r.acct, r.st, r.root, r.sroots, r.lv_storage,
                    r.lv_account, f"step {step}: {name}")
        if step % 3 == 2:
            refs, lens, roots, counts = eng.subtree_roots()
            assert eng.finish_top(refs, lens, roots, counts) == r.root, name
