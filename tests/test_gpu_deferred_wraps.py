"""Deferred extension wraps (plain-root calls) on hand-made trie shapes.

In a plain-root call a hashed, non-root branch at depth d whose parent
junction sits at P < d - 1 is parked by the branch kernels and wrapped into
its extension node by k_branch_wrap at the end of the level. The
states here choose the hashed keys directly, so that the level under test
holds exactly the wraps the case names: one in a wave at a given position,
a whole level of them over a chunk boundary, none at all, the wide classes
of the split hash kernel, an inline branch (which must stay inline), and
roots under extensions (never deferred: P = -1).

Every case runs under the gate configurations of test_gpu_pipeline_gates.py
plus SRE_NO_DEFER_WRAP=1, which forces every wrap inline. Only levels on
the class partition defer, so under the base configuration (production
gates) levels this small wrap inline, and the SRE_CLS_MIN=1 configurations
are the ones that reach the job queue and k_branch_wrap. The reference is
the C oracle; roots, per-account storage roots and the shard decomposition
are compared bit for bit.

There is no counter case: the C ABI has no getter for deferred / inline wrap
counts (tests/test_abi_cpu.py pins the number of exported functions), so
that the deferred path ran is shown by the kernel traces under profiles/, not
here.
"""
import functools
import os

import numpy as np
import pytest

from oracle import bind, pyref
from tests.util import to_arrays

pytestmark = pytest.mark.gpu

CONFIGS = {
    "base": {},
    "cls": {"SRE_CLS_MIN": "1"},
    "cls+chunk": {"SRE_CLS_MIN": "1", "SRE_BR_CHUNK": "256"},
    "split+chunk": {"SRE_CLS_MIN": "1", "SRE_BR_CHUNK": "256",
                    "SRE_NO_FUSED": "1"},
    "inline+chunk": {"SRE_CLS_MIN": "1", "SRE_BR_CHUNK": "256",
                     "SRE_NO_DEFER_WRAP": "1"},
}
GATE_VARS = ("SRE_CLS_MIN", "SRE_BR_CHUNK", "SRE_NO_FUSED",
             "SRE_NO_DEFER_WRAP")

BIG = (1 << 255) + 12345  # 32-byte value: every leaf is hashed


@pytest.fixture(scope="module", params=list(CONFIGS))
def eng(request):
    for v in GATE_VARS:
        assert v not in os.environ, v
    os.environ.update(CONFIGS[request.param])  # getenv is read per call
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()
    for v in GATE_VARS:
        os.environ.pop(v, None)


# --------------------------------------------------------------------------
# keys
# --------------------------------------------------------------------------

def _key(prefix, tag):
    """32-byte key: the hex nibbles `prefix`, then filler from keccak(tag)."""
    fill = bind.keccak256(repr(tag).encode()).hex()
    return bytes.fromhex((prefix + fill)[:64])


def _fill(n, tag):
    return bind.keccak256(repr(tag).encode()).hex()[:n]


def _acct_keys(n):
    """n account keys, sorted: account i is the i-th of its level."""
    return sorted(_key("", ("acct", i)) for i in range(n))


def _acct(slots):
    return (1, 10 ** 18, pyref.KECCAK_EMPTY, slots)


def _under_extension(tag, d, P, nibs="01", value=BIG):
    """Slots of one storage trie: a branch at depth d with children `nibs`,
    whose parent junction is a two-child branch at depth P (P < d). With
    P < d - 1 the depth-d branch sits under an extension of d - P - 1
    nibbles starting at nibble P + 1. The depth-P branch is the trie's root
    branch (under a root extension when P > 0)."""
    assert 0 <= P < d <= 63
    stem = _fill(d, ("stem", tag))
    slots = {_key(stem + c, (tag, c)): value for c in nibs}
    other = "%x" % (int(stem[P], 16) ^ 8)
    slots[_key(stem[:P] + other, (tag, "other"))] = value
    assert len(slots) == len(nibs) + 1
    return slots


def _no_extension(tag):
    """Slots of one storage trie with a two-child branch at depth 2 whose
    parent is a branch at depth 1, below a root branch at depth 0: no
    extension anywhere."""
    a, b = _fill(2, ("stem", tag))
    b2 = "%x" % (int(b, 16) ^ 8)
    a2 = "%x" % (int(a, 16) ^ 8)
    return {_key(a + b + "0", (tag, 0)): BIG, _key(a + b + "1", (tag, 1)): BIG,
            _key(a + b2, (tag, 2)): BIG, _key(a2, (tag, 3)): BIG}


def _extensions_in(slot_keys):
    """(d, P) of every non-root branch of the trie over the sorted hex keys
    that sits under an extension, from the keys alone."""
    lcp = [-1] + [len(os.path.commonprefix(p))
                  for p in zip(slot_keys, slot_keys[1:])] + [-1]
    out = set()
    for i in range(1, len(slot_keys)):
        d = lcp[i]
        lo = i - 1
        while lcp[lo] >= d:
            lo -= 1
        hi = i + 1
        while lcp[hi] >= d:
            hi += 1
        P = max(lcp[lo], lcp[hi])
        if P >= 0 and d > P + 1:
            out.add((lo, d, P))
    return sorted((d, P) for _, d, P in out)


# --------------------------------------------------------------------------
# states, built and referenced once
# --------------------------------------------------------------------------

N_WAVE = 131  # three waves of level-2 groups, the last one partial


def _one_in_a_wave(pos):
    keys = _acct_keys(N_WAVE)
    accounts = {}
    for i, k in enumerate(keys):
        if i == pos:  # depth-2 branch straight under the depth-0 root branch
            slots = _under_extension(("one", i), 2, 0)
        else:
            slots = _no_extension(("one", i))
        accounts[k] = _acct(slots)
    return accounts


def _all_of_a_level(d):
    """301 storage tries, each with its only deep branch at depth d under an
    extension of 1, 2, 7 or 60 nibbles (d = 62: from = 61, 60, 55, 2;
    d = 61: from = 60, 59, 54, 1)."""
    keys = _acct_keys(301)
    return {k: _acct(_under_extension(("all", d, i), d,
                                      d - 1 - (1, 2, 7, 60)[i % 4]))
            for i, k in enumerate(keys)}


def _none():
    keys = _acct_keys(70)
    return {k: _acct(_no_extension(("none", i))) for i, k in enumerate(keys)}


def _classes():
    """4-, 9- and 16-child branches under extensions (classes 1-3: the split
    k_branch_hash path), and a 2-child branch of inline children under an
    extension, as in test_gpu_adversarial.inline_node_chains: its RLP is
    below 32 bytes, so it is embedded and must take the inline wrap."""
    keys = _acct_keys(8)
    h = "0123456789abcdef"
    shapes = [("c1", 5, 2, h[:4], BIG), ("c2", 6, 1, h[3:12], BIG),
              ("c3", 9, 3, h, BIG), ("c3odd", 8, 3, h, BIG),
              ("c1long", 40, 3, h[2:7], BIG),
              ("inl", 62, 10, "01", 1), ("inl2", 61, 3, "5c", 2),
              ("c0", 4, 0, "29", BIG)]
    return {k: _acct(_under_extension(tag, d, P, nibs, v))
            for k, (tag, d, P, nibs, v) in zip(keys, shapes)}


def _shared(n, share, tag):
    """n keys sharing exactly `share` leading nibbles."""
    stem = _fill(share, ("shared", tag))
    heads = "3a7"[:n]
    return [_key(stem + c, (tag, c)) for c in heads]


def _storage_roots_under_extensions():
    keys = _acct_keys(4)
    shapes = [(2, 1), (3, 1), (2, 5), (3, 5)]
    return {k: _acct({s: BIG for s in _shared(n, share, ("sroot", n, share))})
            for k, (n, share) in zip(keys, shapes)}


def _account_root_under_extension(n, share):
    return {k: _acct({_key("", ("slot", n, share)): 7})
            for k in _shared(n, share, ("aroot", n, share))}


STATES = {
    **{f"one_at_{p}": functools.partial(_one_in_a_wave, p)
       for p in (0, 63, 64, N_WAVE - 1)},
    "all_d62": functools.partial(_all_of_a_level, 62),
    "all_d61": functools.partial(_all_of_a_level, 61),
    "none": _none,
    "classes": _classes,
    "storage_roots": _storage_roots_under_extensions,
    **{f"account_root_{n}x{share}":
       functools.partial(_account_root_under_extension, n, share)
       for n in (2, 3) for share in (1, 5)},
}


class Ref:
    def __init__(self, name):
        self.accounts = STATES[name]()
        self.acct, self.st = to_arrays(self.accounts)
        self.root = bind.state_root(self.acct, self.st)
        self.sroots = bind.storage_roots(self.acct, self.st)
        self.subtree = bind.subtree_roots(self.acct, self.st)

    def storage_extensions(self):
        """Per account, in key order: [(d, P)] of its wrapped branches."""
        return [_extensions_in(sorted(s.hex() for s in a[3]))
                for _, a in sorted(self.accounts.items())]


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return Ref(name)


# --------------------------------------------------------------------------
# the shapes are what the cases say they are (from the keys alone)
# --------------------------------------------------------------------------

@pytest.mark.parametrize("pos", [0, 63, 64, N_WAVE - 1])
def test_shape_one_in_a_wave(pos):
    ext = ref_of(f"one_at_{pos}").storage_extensions()
    assert [i for i, e in enumerate(ext) if e] == [pos]
    assert ext[pos] == [(2, 0)]


@pytest.mark.parametrize("d", [62, 61])
def test_shape_all_of_a_level(d):
    ext = ref_of(f"all_d{d}").storage_extensions()
    assert len(ext) == 301 and 301 % 64 and 301 % 256
    assert all(len(e) == 1 and e[0][0] == d for e in ext)
    assert {d - P - 1 for e in ext for _, P in e} == {1, 2, 7, 60}
    assert {(P + 1) & 1 for e in ext for _, P in e} == {0, 1}


def test_shape_none_and_classes():
    assert not any(ref_of("none").storage_extensions())
    assert sorted(e[0] for e in ref_of("classes").storage_extensions()) == \
        sorted([(5, 2), (6, 1), (9, 3), (8, 3), (40, 3), (62, 10), (61, 3),
                (4, 0)])


# --------------------------------------------------------------------------
# engine vs oracle
# --------------------------------------------------------------------------

@pytest.mark.parametrize("state", list(STATES))
def test_roots(eng, state):
    r = ref_of(state)
    eng.upload(r.acct, r.st)
    assert eng.root() == r.root, state
    got = eng.storage_roots(len(r.acct))
    bad = np.nonzero((got != r.sroots).any(axis=1))[0]
    assert not len(bad), \
        f"{state}: storage root of account {bytes(r.acct[bad[0]]['key']).hex()}"
    refs, lens, roots, counts = eng.subtree_roots()
    assert np.array_equal(lens, r.subtree[1]), state
    assert np.array_equal(refs, r.subtree[0]), state
    assert np.array_equal(roots, r.subtree[2]), state
    assert eng.finish_top(refs, lens, roots, counts) == r.root, state
    assert eng.root() == r.root, f"{state}, second call"


@pytest.mark.parametrize("state", ["one_at_64", "all_d62", "classes"])
def test_updates_mode_still_matches(eng, state):
    """An updates-mode call on the same state keeps every wrap inline."""
    r = ref_of(state)
    eng.upload(r.acct, r.st)
    root, rows = eng.root_with_updates()
    want_root, want_rows = bind.state_root_with_updates(r.acct, r.st)
    assert root == want_root == r.root, state
    assert rows.tobytes() == want_rows.tobytes(), state
