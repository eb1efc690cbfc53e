"""Level members read in place: recs[idx[p]] instead of a dense copy.

The level select lists the members' slots (k_level_gather -> idx, gs) and
every consumer (k_branch_assemble, k_branch_fused1, k_emit_updates,
k_proof_grab, k_capture_L) reads member p as recs[idx[p]], while the same
level's new branches are stored over their first members. The shapes here
are the smallest at which that addressing can go wrong:

- sparse members: a level whose members are placed branches more than 1024
  leaves apart, so each sits in another 1024-slot wave span of the select;
  one group reaches over three spans, one group's two members are the first
  and the last slot the level selects;
- neighbours across pipeline stages: groups whose records share a 128-B line
  while one is written and the other read, by different kernels on
  different streams (chunk edge under SRE_BR_CHUNK=256, fused | split class
  edge). A class-1 group has at least four members, so "split first" puts
  the first slots four apart, not two; its last member's record and the
  fused group's first still share a line;
- one slot that is a member, is overwritten, and is a member again, for five
  consecutive levels (the staircases of test_gpu_inplace_levels.py);
- branches whose parent depth P is 6, 7, 8, 9, with and without an extension
  over nibbles 7|8: the edge of a key's first four bytes. branch_tail reads
  the child nibble at P from the key today; a record that carried those
  bytes (measured, left out: DESIGN.md §9b.2) would switch source here;
- the other consumers on one combined state: TrieUpdates rows, multiproofs,
  retained cell tops re-seeded into a new branch.

Every shape property is asserted in Python from the sorted keys before a
root is trusted; every case compares root and per-account storage roots
with the C oracle and stats()["branch_count"] / ["levels"] with what the
keys predict, under the default gates and under SRE_CLS_MIN=1
SRE_BR_CHUNK=256.
"""
import functools
import os

import numpy as np
import pytest

from oracle import bind, pyref
from tests import dense_cells as dc
from tests.test_gpu_incremental import _arrays_of, _mk_delta
from tests.test_gpu_inplace_levels import (_check_root, _members, stair_accounts,
                                           stair_storage, STAIR_J)
from tests.test_gpu_pipeline_gates import _branch_levels
from tests.test_gpu_proof import _replay
from tests.util import to_arrays

pytestmark = pytest.mark.gpu

KE = pyref.KECCAK_EMPTY
CONFIGS = {
    "base": {},
    "cls+chunk": {"SRE_CLS_MIN": "1", "SRE_BR_CHUNK": "256"},
}
SPAN = 1024   # slots per wave of the level select
CHUNK = 256   # SRE_BR_CHUNK of the lowered configuration
REC = 48      # sizeof(node_rec)
LINE = 128


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
# keys
# --------------------------------------------------------------------------

def _key(prefix, tag):
    """`prefix` nibbles, then the nibbles of keccak(tag)."""
    n = dc.nibbles(bind.keccak256(b"lvidx" + tag))
    n[:len(prefix)] = prefix
    return dc._from_nibbles(n)


def _akey(i):
    """Account keys that sort by i (top nibble 1, so they sit between the
    boundary families of top nibbles 0 and 7)."""
    return bytes([0x10, i]) + bind.keccak256(b"lvidx-acct%d" % i)[2:]


def _holder(i, slots):
    return {_akey(i): (1, 1000 + i, KE, {k: 1 + j for j, k in enumerate(slots)})}


MEMBER_LEAVES = 1030  # > SPAN: consecutive members lie in different spans


def sparse_slot_keys():
    """Depth-1 branches 0 and 3 over depth-2 subtrees of MEMBER_LEAVES random
    keys each: (0,1) (0,5) (0,9) | (3,2) (3,3). The root branch has the two
    members 0 and 3."""
    keys = []
    for a, b in ((0, 1), (0, 5), (0, 9), (3, 2), (3, 3)):
        keys += [_key([a, b], b"sp%d/%d/%d" % (a, b, i))
                 for i in range(MEMBER_LEAVES)]
    return keys


def sparse_state():
    return _holder(0, sparse_slot_keys())


N_STAGE_GROUPS = 800
STAGE_SIZES = {256: 4, 767: 4}  # class-1 groups; every other group: 2 leaves


def stage_slot_keys():
    """Depth-3 group k has the prefix (k >> 8, k >> 4 & 15, k & 15) and the
    children 0, 1 (, 2, 3)."""
    keys = []
    for k in range(N_STAGE_GROUPS):
        p = [k >> 8, (k >> 4) & 15, k & 15]
        keys += [_key(p + [c], b"stg%d/%d" % (k, c))
                 for c in range(STAGE_SIZES.get(k, 2))]
    return keys


def stage_state():
    # a two-leaf trie in front shifts every slot by two: see test_stage_shape
    acc = _holder(0, [_key([0], b"front0"), _key([1], b"front1")])
    acc.update(_holder(1, stage_slot_keys()))
    return acc


BOUNDARY_P = (6, 7, 8, 9)
BOUNDARY_EXT = (0, 2)  # nibbles of extension between the two branches
BOUNDARY_TOPS = (0, 7, 15)


def boundary_keys(tops=BOUNDARY_TOPS):
    """Per (top nibble, P, ext) one family of three keys under the P-nibble
    prefix (top, f, 0, ...): a leaf A = prefix+1 and two leaves prefix+2+
    (ext nibbles of 5)+3 / +4. The family has a branch at depth P and one at
    depth P+1+ext whose parent depth is P; with ext = 2 an extension covers
    nibbles P+1, P+2 between them (7|8 for P = 6)."""
    keys = []
    for t in tops:
        for f, (p, ext) in enumerate((p, e) for p in BOUNDARY_P
                                     for e in BOUNDARY_EXT):
            pre = [t, f] + [0] * (p - 2)
            tag = b"bd%d/%d/%d" % (t, p, ext)
            keys.append(_key(pre + [1], tag + b"A"))
            keys.append(_key(pre + [2] + [5] * ext + [3], tag + b"B"))
            keys.append(_key(pre + [2] + [5] * ext + [4], tag + b"C"))
    return keys


def boundary_storage():
    return _holder(0, boundary_keys())


def boundary_accounts():
    return {k: (i, 10 ** 12 + i, KE, {}) for i, k in enumerate(boundary_keys())}


# one 4-nibble group of the account trie for the retained-row case: cell
# CELL_B holds the P = 6 boundary family, its sibling cells plain accounts
GROUP = 0x7F3A
CELL_B, CELL_N, CELL_M = GROUP << 4 | 0x2, GROUP << 4 | 0x3, GROUP << 4 | 0xC


def _cell_prefix(c):
    return [(c >> s) & 0xF for s in (16, 12, 8, 4, 0)]


def combined_state():
    """Sparse storage members, the boundary families as accounts and as a
    storage trie, and the cell group of the retained-row case."""
    acc = boundary_accounts()
    acc.update(_holder(0, sparse_slot_keys()))
    acc.update(_holder(1, boundary_keys()))
    pre = _cell_prefix(CELL_B)
    fam = [_key(pre + [1], b"cbA"),             # branch at depth 5 ...
           _key(pre + [2, 6, 3], b"cbB"),       # ... and at depth 7, P = 5
           _key(pre + [2, 6, 4], b"cbC")]
    for i, k in enumerate(fam):
        acc[k] = (i, 5 * 10 ** 11 + i, KE, {})
    for c in (CELL_N, CELL_M):
        for i in range(4):
            acc[dc.key_in(c, b"cn%d" % i)] = (i, 3 * 10 ** 11 + i, KE, {})
    return acc


STATES = {
    "sparse": sparse_state,
    "stage": stage_state,
    "stair_storage": stair_storage,
    "stair_accounts": stair_accounts,
    "boundary_storage": boundary_storage,
    "boundary_accounts": boundary_accounts,
    "combined": combined_state,
}


class Ref:
    def __init__(self, name):
        self.accounts = STATES[name]()
        self.acct, self.st = to_arrays(self.accounts)
        self.root = bind.state_root(self.acct, self.st)
        self.sroots = bind.storage_roots(self.acct, self.st)
        ak = self.st["acct_key"].tobytes()
        sk = self.st["slot_key"].tobytes().hex()
        self.st_tries, prev = [], None  # (first entry, sorted hex keys)
        for i in range(len(self.st)):
            a = ak[32 * i:32 * i + 32]
            if a != prev:
                self.st_tries.append((i, []))
                prev = a
            self.st_tries[-1][1].append(sk[64 * i:64 * i + 64])
        raw = self.acct["key"].tobytes().hex()
        self.ac_tries = [(0, [raw[i:i + 64] for i in range(0, len(raw), 64)])]
        self.lv_storage = _branch_levels(k for _, k in self.st_tries)
        self.lv_account = _branch_levels(k for _, k in self.ac_tries)

    @functools.cached_property
    def st_members(self):
        return _members(self.st_tries)

    @functools.cached_property
    def ac_members(self):
        return _members(self.ac_tries)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return Ref(name)


def _same_line(a, b):
    """Do the records of slots a < b touch a common 128-B line?"""
    return (a * REC + REC - 1) // LINE == (b * REC) // LINE


def _parent_depths(members):
    """{(depth, first slot): parent depth} of every branch that is not a
    root: the deepest level above it that lists its slot as a member."""
    out = {}
    for d, groups in members.items():
        for m in groups:
            up = [p for p in members if p < d and
                  any(m[0] in g for g in members[p])]
            if up:
                out[(d, m[0])] = max(up)
    return out


# --------------------------------------------------------------------------
# the shape properties, from the sorted keys alone
# --------------------------------------------------------------------------

def test_sparse_shape():
    r = ref_of("sparse")
    assert len(r.st) == 5 * MEMBER_LEAVES and r.st_tries[0][0] == 0
    lv = r.st_members
    g1 = sorted(lv[1])
    assert g1 == [[0, MEMBER_LEAVES, 2 * MEMBER_LEAVES],
                  [3 * MEMBER_LEAVES, 4 * MEMBER_LEAVES]]
    slots = [s for g in g1 for s in g]
    # every member is a placed branch covering more than a span of leaves ...
    for s, nxt in zip(slots, slots[1:] + [len(r.st)]):
        assert nxt - s > SPAN
        assert any(s == g[0] for g in lv[2]), s
    # ... so no two members share a span; group 0 reaches two spans further
    assert len({s // SPAN for s in slots}) == len(slots)
    assert g1[0][-1] // SPAN == g1[0][0] // SPAN + 2
    # the root branch: first and last slot that its level selects
    assert lv[0] == [[0, 3 * MEMBER_LEAVES]]
    assert 3 * MEMBER_LEAVES // SPAN == 3


def test_stage_shape():
    r = ref_of("stage")
    off, keys = r.st_tries[1]
    assert off == 2 and len(keys) == 2 * N_STAGE_GROUPS + 4
    assert set(r.st_members) == {0, 1, 2, 3}  # the front trie: depth 0 only
    g3 = sorted(r.st_members[3])
    assert len(g3) == N_STAGE_GROUPS
    assert [len(g) for g in g3] == [STAGE_SIZES.get(k, 2)
                                    for k in range(N_STAGE_GROUPS)]
    first = [g[0] for g in g3]
    # fused last of chunk 0 | split first of chunk 1, first slots s, s + 2
    a, b = CHUNK - 1, CHUNK
    assert (len(g3[a]), len(g3[b])) == (2, 4) and first[b] == first[a] + 2
    assert _same_line(first[a], first[b])
    # fused | fused over the edge of chunks 1 and 2
    a, b = 2 * CHUNK - 1, 2 * CHUNK
    assert (len(g3[a]), len(g3[b])) == (2, 2) and first[b] == first[a] + 2
    assert _same_line(first[a], first[b])
    # split last of chunk 2 | fused first of chunk 3: four members, so the
    # first slots are four apart; the split group's last member (read by
    # k_branch_assemble) shares a line with the slot the fused kernel writes
    a, b = 3 * CHUNK - 1, 3 * CHUNK
    assert (len(g3[a]), len(g3[b])) == (4, 2) and first[b] == first[a] + 4
    assert g3[a][-1] + 1 == first[b] and _same_line(g3[a][-1], first[b])


@pytest.mark.parametrize("name,which", [("stair_storage", "st_members"),
                                        ("stair_accounts", "ac_members")])
def test_stair_shape(name, which):
    lv = getattr(ref_of(name), which)
    # some slot starts a group at five consecutive depths: a member at d, it
    # is overwritten by d's branch and is a member again at d - 1
    best = 0
    for s in {g[0] for groups in lv.values() for g in groups}:
        run = 0
        for d in range(63, -1, -1):
            starts = any(g[0] == s for g in lv.get(d, ()))
            run = run + 1 if starts else 0
            best = max(best, run)
    assert best >= 5, best
    assert {63 - j for j in STAIR_J} <= set(lv)


@pytest.mark.parametrize("name,which", [("boundary_storage", "st_members"),
                                        ("boundary_accounts", "ac_members")])
def test_boundary_shape(name, which):
    lv = getattr(ref_of(name), which)
    parents = _parent_depths(lv)
    for ext in BOUNDARY_EXT:
        for p in BOUNDARY_P:
            n = sum(1 for (d, _), up in parents.items()
                    if up == p and d == p + 1 + ext)
            assert n == len(BOUNDARY_TOPS), (p, ext, n)
    if which == "ac_members":
        tops = {int(k[0], 16) for k in ref_of(name).ac_tries[0][1]}
        assert tops == set(BOUNDARY_TOPS)


# --------------------------------------------------------------------------
# roots and counters
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(STATES))
def test_roots(eng, name):
    r = ref_of(name)
    eng.upload(r.acct, r.st)
    _check_root(eng, r.acct, r.st, r.root, r.sroots, r.lv_storage,
                r.lv_account, name)


@pytest.mark.parametrize("name", ["boundary_accounts", "combined"])
def test_subtree_roots(eng, name):
    """Shard decomposition: the account pass indexes child_refs / seg_roots
    by the key's top nibble (0, 7 and 15 here)."""
    r = ref_of(name)
    tops = {k[0] >> 4 for k in r.accounts}
    assert {0, 7, 15} <= tops
    eng.upload(r.acct, r.st)
    refs, lens, roots, counts = eng.subtree_roots()
    want = bind.subtree_roots(r.acct, r.st)
    assert np.array_equal(lens, want[1]), name
    assert np.array_equal(refs, want[0]), name
    assert np.array_equal(roots, want[2]), name
    assert eng.finish_top(refs, lens, roots, counts) == r.root, name
    stats = eng.stats()
    sub = {d: v for d, v in r.lv_account.items() if d > 0}
    assert stats["levels"] == len(r.lv_storage) + len(sub), name
    assert stats["branch_count"] == \
        sum(v[0] for v in r.lv_storage.values()) + \
        sum(v[0] for v in sub.values()), name


# --------------------------------------------------------------------------
# the other consumers, on the combined state
# --------------------------------------------------------------------------

def test_combined_updates(eng):
    r = ref_of("combined")
    want_root, want_rows = bind.state_root_with_updates(r.acct, r.st)
    eng.upload(r.acct, r.st)
    root, rows = eng.root_with_updates()
    assert root == want_root == r.root
    assert len(rows) == len(want_rows), (len(rows), len(want_rows))
    ga = rows.view(np.uint8).reshape(len(rows), -1)
    wa = want_rows.view(np.uint8).reshape(len(want_rows), -1)
    bad = np.nonzero((ga != wa).any(axis=1))[0]
    assert not len(bad), f"row {bad[0]}: engine={rows[bad[0]]} " \
                         f"oracle={want_rows[bad[0]]}"


def test_combined_proofs(eng):
    r = ref_of("combined")
    eng.upload(r.acct, r.st)
    # account: the deepest leaf of the P = 9 family under top nibble 15
    akey = max(k for k in boundary_keys())
    nodes, = eng.account_proof([akey])
    assert _replay(nodes, akey, r.root) is not None
    # storage: a slot of the last sparse member (the level's last slot)
    holder, slot = _akey(0), max(sparse_slot_keys())
    (sroot,), (snodes,) = eng.storage_proof([holder], [slot])
    i = [bytes(k) for k in r.acct["key"]].index(holder)
    assert sroot == bytes(r.sroots[i])
    assert _replay(snodes, slot, sroot) is not None
    # and across the 7|8 boundary of the storage copy of the families
    holder, slot = _akey(1), min(boundary_keys())
    (sroot,), (snodes,) = eng.storage_proof([holder], [slot])
    assert _replay(snodes, slot, sroot) is not None


def test_combined_retained_rows(eng):
    """The boundary cell stays clean over two deltas that dirty a sibling
    cell: its retained record is re-seeded and becomes the first member of
    the rebuilt depth-4 branch."""
    acc = {k: list(v) for k, v in combined_state().items()}
    cells = sorted({dc.cell(k) for k in acc if dc.group(k) == GROUP})
    assert cells == [CELL_B, CELL_N, CELL_M]  # CELL_B is the first member
    acct, st = _arrays_of(acc)
    eng.upload(acct, st)
    assert eng.root_retaining() == bind.state_root(acct, st)
    deltas = [
        [dc.mod(acc, dc.keys_of(acc, CELL_N)[0])],
        [dc.ins(dc.key_in(CELL_M, b"new")), dc.dele(dc.keys_of(acc, CELL_N)[1])],
    ]
    for step, rows in enumerate(deltas):
        assert all(dc.cell(row[0]) != CELL_B for row in rows)
        dc.apply_rows(acc, rows)
        d, s = _mk_delta(rows, [])
        assert eng.incremental_root(d, s) == \
            bind.state_root(*_arrays_of(acc)), f"delta {step}"
        assert eng.incremental_counters()["seeded"] > 0, f"delta {step}"
    acct, st = _arrays_of(acc)
    eng.upload(acct, st)
    assert eng.root() == bind.state_root(acct, st)
