"""Level nodes kept in place by interval start (recs[s] / depths[s]).

A level's input is selected straight from the in-place slots
(k_level_count / k_level_gather), group starts come from the same sweep
(lcp[s] < d), and a level's new branches are written back over their first
child's slot (k_place_nodes). The shapes here are the smallest at which
those movers can go wrong:

- segments and groups on the edges of the sweep's units. The select works in
  1024-slot wave spans of 16-slot lanes and 64-slot rounds; 256 is the
  launch block. Every edge property is asserted in Python, from the sorted
  keys alone and for both 256 and 1024, before any root is trusted;
- one slot overwritten level after level (spine "staircase" tries, with
  extension jumps), in a storage trie and in the account trie;
- single-leaf and two-leaf tries (never selected, or selected once) between
  large ones;
- one chained call sequence on one engine, every step against the oracle, so
  stale state in pooled buffers shows up.

Every case compares the root and the per-account storage roots with the C
oracle and requires stats()["branch_count"] and ["levels"] to equal what the
keys predict (test_gpu_pipeline_gates._branch_levels), under the default
gates and under SRE_CLS_MIN=1 SRE_BR_CHUNK=256.
"""
import functools
import os

import numpy as np
import pytest

from oracle import bind, pyref
from tests import dense_cells as dc
from tests.test_gpu_incremental import _arrays_of, _mk_delta
from tests.test_gpu_pipeline_gates import _branch_levels
from tests.test_gpu_proof import _replay
from tests.util import to_arrays

pytestmark = pytest.mark.gpu

KE = pyref.KECCAK_EMPTY
CONFIGS = {
    "base": {},
    "cls+chunk": {"SRE_CLS_MIN": "1", "SRE_BR_CHUNK": "256"},
}
UNITS = (256, 1024)  # launch block, wave span of the level select


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

def _akey(i):
    """Account keys that sort by i."""
    return (i + 1).to_bytes(2, "big") + bind.keccak256(b"ip-acct%d" % i)[2:]


def _skey(i, j):
    return bind.keccak256(b"ip-slot%d/%d" % (i, j))


def storage_counts(counts):
    """Account i gets counts[i] random slots; entries follow account order."""
    return {_akey(i): (1, 1000 + i, KE,
                       {_skey(i, j): 1 + j + (i << 8) for j in range(c)})
            for i, c in enumerate(counts)}


def account_only(n):
    return {bind.keccak256(b"ip-only%d" % i): (i % 5, 10 ** 9 + i, KE, {})
            for i in range(n)}


def _from_nibbles(n):
    return bytes((n[2 * i] << 4) | n[2 * i + 1] for i in range(32))


# shared nibbles with key 0 drop by more than one at 3->6, 29->37, ...:
# extension nodes between the spine's branches
STAIR_J = [j for j in range(1, 61) if j % 7 not in (4, 5) and not 30 <= j <= 36]


def stair_keys(left):
    """Key j shares exactly 63-j nibbles with key 0. Left spine: key 0 is the
    smallest, so every spine branch starts at slot 0 and is re-placed there
    at every depth while its end grows. Right spine (mirrored): key 0 is the
    largest and each branch lands one slot further left."""
    base = [0x0 if left else 0xF] * 64
    keys = [_from_nibbles(base)]
    for j in STAIR_J:
        n = list(base)
        n[63 - j] = 1 + j % 14 if left else 0xE - j % 14
        keys.append(_from_nibbles(n))
    return keys


def stair_storage():
    acc = storage_counts([1, 0, 2, 0, 3, 1])
    for i, left in ((1, True), (3, False)):
        slots = {k: 1 + j for j, k in enumerate(stair_keys(left))}
        acc[_akey(i)] = (1, 1000 + i, KE, slots)
    return acc


def stair_accounts():
    keys = stair_keys(True) + stair_keys(False)
    return {k: (i, 10 ** 12 + i, KE, {}) for i, k in enumerate(keys)}


MIX = [64, 17, 3, 2, 1, 64, 64, 17, 3, 2, 1, 17]             # 255 entries
MIX4 = [257, 257, 257, 64, 64, 64, 17, 17, 17, 3, 3, 2, 1]   # 1023 entries
assert sum(MIX) == 255 and sum(MIX4) == 1023

STATES = {
    # totals on the unit edges; segments straddle the 256 boundaries
    "st255": lambda: storage_counts(MIX),
    "st256": lambda: storage_counts(MIX + [1]),
    "st257": lambda: storage_counts([257]),  # block 0 inside one segment
    # the 257-slot segment starts on block 0's last lane and holds block 1
    "st513": lambda: storage_counts(MIX + [257, 1]),
    "st1023": lambda: storage_counts(MIX4),
    "st1024": lambda: storage_counts(MIX4 + [1]),
    "st1025": lambda: storage_counts(MIX4 + [2]),  # trie across the span edge
    # starts on span 0's last lane and holds all of span 1
    "st_span_inside": lambda: storage_counts(MIX4 + [2100, 2]),
    # single- and two-leaf tries between large ones: whole blocks and whole
    # spans without a member at any level
    "st_gap256": lambda: storage_counts([257] + [1] * 600 + [2] * 5 + [257]),
    "st_gap1024": lambda: storage_counts([1100] + [1] * 2100 + [2] * 10
                                         + [1100, 1, 2]),
    "ac255": lambda: account_only(255),
    "ac256": lambda: account_only(256),
    "ac257": lambda: account_only(257),
    "ac1023": lambda: account_only(1023),
    "ac1025": lambda: account_only(1025),
    "ac3100": lambda: account_only(3100),
    "stair_storage": stair_storage,
    "stair_accounts": stair_accounts,
}


class Ref:
    def __init__(self, name):
        self.acct, self.st = to_arrays(STATES[name]())
        self.root = bind.state_root(self.acct, self.st)
        self.sroots = bind.storage_roots(self.acct, self.st)
        ak = self.st["acct_key"].tobytes()
        sk = self.st["slot_key"].tobytes().hex()
        # storage tries as (first entry, sorted hex keys), in entry order
        self.st_tries, prev = [], None
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


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return Ref(name)


# --------------------------------------------------------------------------
# the edge properties, from the sorted keys alone
# --------------------------------------------------------------------------

def _members(tries):
    """{depth: [member slots of one branch node, ...]}: a member's slot is
    the entry index of its first key, which is where its record lives."""
    levels = {}
    for off, keys in tries:
        branches = {a[:len(os.path.commonprefix((a, b)))]
                    for a, b in zip(keys, keys[1:])}
        groups = {}
        for i, k in enumerate(keys):
            for n in range(64):
                if k[:n] in branches and \
                        (i == 0 or keys[i - 1][:n + 1] != k[:n + 1]):
                    groups.setdefault(k[:n], []).append(off + i)
        for p, m in groups.items():
            levels.setdefault(len(p), []).append(m)
    return levels


def _edge_properties(levels, unit):
    first_on_last_lane = spans_two = empty_between = False
    for groups in levels.values():
        for m in groups:
            first_on_last_lane |= m[0] % unit == unit - 1
            spans_two |= m[0] // unit != m[-1] // unit
        blocks = sorted({s // unit for m in groups for s in m})
        empty_between |= any(b - a > 1 for a, b in zip(blocks, blocks[1:]))
    return first_on_last_lane, spans_two, empty_between


def test_shapes_reach_the_edges():
    got = {u: [False] * 3 for u in UNITS}
    for name in STATES:
        r = ref_of(name)
        for tries, lv in ((r.st_tries, r.lv_storage),
                          (r.ac_tries, r.lv_account)):
            members = _members(tries)
            # the member model and the counter model agree on the groups
            assert {d: len(g) for d, g in members.items()} == \
                {d: v[0] for d, v in lv.items()}, name
            for u in UNITS:
                got[u] = [a or b for a, b in
                          zip(got[u], _edge_properties(members, u))]
    for u in UNITS:
        assert got[u] == [True] * 3, \
            (u, "first member on a unit's last lane / group spanning two "
                "units / empty unit between populated ones", got[u])
    # the named placements
    assert ref_of("st513").st_tries[-2][0] == 255
    assert ref_of("st_span_inside").st_tries[-2][0] == 1023
    assert len(ref_of("st1025").st_tries[-1][1]) == 2
    assert ref_of("st1025").st_tries[-1][0] == 1023
    # staircases: a branch at almost every depth, slot 0 placed again each time
    for name, lv in (("stair_storage", ref_of("stair_storage").lv_storage),
                     ("stair_accounts", ref_of("stair_accounts").lv_account)):
        assert len(lv) >= len(STAIR_J), name
        assert {63 - j for j in STAIR_J} <= set(lv), name


# --------------------------------------------------------------------------
# roots and counters
# --------------------------------------------------------------------------

def _check_root(eng, acct, st, root, sroots, lv_storage, lv_account, tag):
    assert eng.root() == root, tag
    stats = eng.stats()
    assert stats["levels"] == len(lv_storage) + len(lv_account), tag
    assert stats["branch_count"] == \
        sum(v[0] for v in lv_storage.values()) + \
        sum(v[0] for v in lv_account.values()), tag
    got = eng.storage_roots(len(acct))
    bad = np.nonzero((got != sroots).any(axis=1))[0]
    assert not len(bad), f"{tag}: storage root of account {bad[0]}"


@pytest.mark.parametrize("name", list(STATES))
def test_roots(eng, name):
    r = ref_of(name)
    eng.upload(r.acct, r.st)
    _check_root(eng, r.acct, r.st, r.root, r.sroots, r.lv_storage,
                r.lv_account, name)


def _levels_of(acct, st):
    by_acct = {}
    ak, sk = st["acct_key"].tobytes(), st["slot_key"].tobytes().hex()
    for i in range(len(st)):
        by_acct.setdefault(ak[32 * i:32 * i + 32], []).append(
            sk[64 * i:64 * i + 64])
    raw = acct["key"].tobytes().hex()
    return (_branch_levels(by_acct.values()),
            _branch_levels([[raw[i:i + 64] for i in range(0, len(raw), 64)]]))


def test_chained_calls_on_one_engine(eng):
    acc = dc.build_state(scale=0.55, slots=True)
    acct, st = _arrays_of(acc)
    want, want_rows = bind.state_root_with_updates(acct, st)
    sroots = bind.storage_roots(acct, st)
    lvs, lva = _levels_of(acct, st)
    eng.upload(acct, st)
    _check_root(eng, acct, st, want, sroots, lvs, lva, "root")

    root, rows = eng.root_with_updates()
    assert root == want
    assert len(rows) == len(want_rows)
    assert rows.tobytes() == want_rows.tobytes(), "update rows"

    akeys = [bytes(k) for k in acct["key"]]
    targets = [akeys[0], akeys[len(akeys) // 2], akeys[-1],
               bind.keccak256(b"ip-absent")]
    items = sorted(
        (pyref.nibbles_of(k), pyref.account_value(
            int(a["nonce"]), int.from_bytes(bytes(a["balance"]), "big"),
            bytes(r), bytes(a["code_hash"])))
        for k, a, r in zip(akeys, acct, sroots))
    proofs = eng.account_proof(targets)
    with pyref.accelerated(bind.keccak256):
        for t, nodes in zip(targets, proofs):
            ref_nodes = []
            pyref._collect_proof(items, 0, pyref.nibbles_of(t), True,
                                 ref_nodes)
            assert nodes == ref_nodes, f"account proof {t.hex()}"
            assert (_replay(nodes, t, want) is not None) == (t in akeys)

    assert eng.root_retaining() == want
    big = dc.keys_of(acc, dc.FULL_BIG)
    deltas = [
        ([dc.mod(acc, dc.deep_key(acc, dc.FULL_BIG))], []),
        ([dc.mod(acc, dc.keys_of(acc, dc.LONE)[0]), dc.ins(dc.key_after(big[0]))],
         [(big[1], bind.keccak256(b"ip-new-slot"), 77)]),
    ]
    for step, (drows, dstrows) in enumerate(deltas):
        dc.apply_rows(acc, drows, dstrows)
        d, s = _mk_delta(drows, dstrows)
        assert eng.incremental_root(d, s) == \
            bind.state_root(*_arrays_of(acc)), f"delta {step}"
        assert eng.incremental_counters()["seeded"] > 0, f"delta {step}"

    acct, st = _arrays_of(acc)
    lvs, lva = _levels_of(acct, st)
    _check_root(eng, acct, st, bind.state_root(acct, st),
                bind.storage_roots(acct, st), lvs, lva, "root after deltas")
