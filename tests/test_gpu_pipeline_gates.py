"""The size-gated branch pipeline on test-sized states.

The class partition (k_class_hist / k_class_scatter, the perm / cinv
indirection), the fused one-block branch kernel and the chunked two-stream
ping-pong only engage at >= 16384 groups per level and > 16 Mi groups per
level. SRE_CLS_MIN and SRE_BR_CHUNK lower those gates (read per call, like
SRE_ST_SMALL_MIN in test_gpu_smallmerge.py) so that adversarial shapes, the
RLP boundary corpora and small generated states run through them — for the
root, per-account storage roots, the shard decomposition, TrieUpdates rows
(the d_perm / urowidx path) and multiproofs (the cinv path).

A gate that silently stays on the old path would prove nothing, so every
call's path counters (sre_get_path_counters) must EQUAL what the trie's
shape predicts: the number of branch nodes per depth, and how many of them
have at most three children, computed here from the keys alone.

Proof references come from pyref's proof walker. Its pure-Python keccak
makes sixteen walks over a few thousand accounts take minutes, so for the
duration of the reference computation (pyref.accelerated) the primitive is
the C oracle's keccak256 (pinned against pyref's in test_oracle_cpu.py) and the
per-account storage roots are taken from the C oracle (pinned against
pyref's on these corpora in test_rlp_corpus_cpu.py / test_oracle_*).
"""
import functools
import os

import numpy as np
import pytest

from oracle import bind, pyref
from reth_amd import gen
from tests import rlp_corpus as rc
from tests import test_gpu_adversarial as adv
from tests.test_gpu_proof import _replay
from tests.util import random_accounts, to_arrays

pytestmark = pytest.mark.gpu

DEFAULT_CLS_MIN = 1 << 14
DEFAULT_CHUNK = 16 << 20

CONFIGS = {
    "base": {},
    "cls": {"SRE_CLS_MIN": "1"},
    "cls+chunk": {"SRE_CLS_MIN": "1", "SRE_BR_CHUNK": "256"},
    "split+chunk": {"SRE_CLS_MIN": "1", "SRE_BR_CHUNK": "256",
                    "SRE_NO_FUSED": "1"},
    "chunk-only": {"SRE_BR_CHUNK": "256"},
    # production class gate; only the chunk is lowered
    "natural": {"SRE_BR_CHUNK": "4096"},
}
GATE_VARS = ("SRE_CLS_MIN", "SRE_BR_CHUNK", "SRE_NO_FUSED")


def _account_grid_all():
    accounts = []
    for nl in range(9):
        accounts += rc.account_leaf_grid(nl)[0]
    return accounts


STATES = {
    "deep_shared_prefixes": adv.deep_shared_prefixes,
    "full_sibling_fan": adv.full_sibling_fan,
    "ragged_storage": adv.ragged_storage,
    "value_rlp_boundaries": adv.value_rlp_boundaries,
    "inline_node_chains": adv.inline_node_chains,
    "storage_leaf_grid": lambda: rc.storage_leaf_grid()[0],
    "account_leaf_grid": _account_grid_all,
    "branch_lengths": lambda: rc.branch_length_state()[0],
    "single_nibble_256": lambda: list(random_accounts(
        trial=7, n=256, single_nibble=True).items()),
    "gen3000x8": (3000, 8),
    "gen20000x8": (20000, 8),
}
SMALL = [s for s in STATES if s != "gen20000x8"]
# states wide enough that every lowered gate changes the path taken
WIDE = ("storage_leaf_grid", "branch_lengths", "gen3000x8")
COMBOS = [(c, s) for c in CONFIGS if c != "natural" for s in SMALL] + \
    [("natural", "gen20000x8")]


@pytest.fixture(scope="module")
def cfg(request):
    name = request.param
    for v in GATE_VARS:
        assert v not in os.environ, v
    os.environ.update(CONFIGS[name])  # getenv is read per call
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield name, e
    e.close()
    for v in GATE_VARS:
        os.environ.pop(v, None)


both = pytest.mark.parametrize("cfg,state", COMBOS, indirect=["cfg"],
                               ids=[f"{c}-{s}" for c, s in COMBOS])


# --------------------------------------------------------------------------
# what the counters must say: branch nodes per depth from the keys alone
# --------------------------------------------------------------------------

def _branch_levels(tries):
    """tries: iterable of sorted hex-key lists, one per trie. Returns
    {depth: [branch nodes, branch nodes with <= 3 children]} summed over
    the tries — a level of the engine's pass is one depth, a group one
    branch node."""
    levels = {}
    for keys in tries:
        kids = {}
        for a, b in zip(keys, keys[1:]):
            n = len(os.path.commonprefix((a, b)))
            kids.setdefault(a[:n], set()).update((a[n], b[n]))
        for prefix, nibs in kids.items():
            lv = levels.setdefault(len(prefix), [0, 0])
            lv[0] += 1
            lv[1] += len(nibs) <= 3
    return levels


def _expect(passes, cfg_name):
    """passes: [(levels, fused_allowed)]. The counters a call must report
    under the named configuration."""
    env = CONFIGS[cfg_name]
    cls_min = int(env.get("SRE_CLS_MIN", DEFAULT_CLS_MIN))
    chunk = int(env.get("SRE_BR_CHUNK", DEFAULT_CHUNK))
    no_fused = "SRE_NO_FUSED" in env
    out = {"class_levels": 0, "fused_groups": 0, "chunks": 0,
           "pipe2_levels": 0}
    for levels, fused_allowed in passes:
        for n, n0 in levels.values():
            out["chunks"] += -(-n // chunk)
            out["pipe2_levels"] += n > chunk
            if n >= cls_min:
                out["class_levels"] += 1
                if fused_allowed and not no_fused:
                    out["fused_groups"] += n0
    return out


# --------------------------------------------------------------------------
# per-state references, computed once and shared by every configuration
# --------------------------------------------------------------------------

def _spread(n, k):
    return sorted({int(i) for i in np.linspace(0, n - 1, min(n, k))})


def _near_miss(key, present):
    k = key[:31] + bytes([key[31] ^ 1])
    return None if k in present else k


class Ref:
    """One state's arrays and references; each part is computed on first
    use, so a test pays only for what it compares against."""

    def __init__(self, name):
        spec = STATES[name]
        if isinstance(spec, tuple):
            self.acct, self.st = gen.gen_state_numpy(*spec,
                                                     bind.keccak256_batch)
        else:
            self.acct, self.st = to_arrays(dict(spec()))
        raw = self.acct["key"].tobytes()
        self.akeys = [raw[i:i + 32] for i in range(0, len(raw), 32)]

    @functools.cached_property
    def root(self):
        return bind.state_root(self.acct, self.st)

    @functools.cached_property
    def sroots(self):
        return bind.storage_roots(self.acct, self.st)

    @functools.cached_property
    def subtree(self):
        return bind.subtree_roots(self.acct, self.st)

    @functools.cached_property
    def updates(self):
        return bind.state_root_with_updates(self.acct, self.st)

    @functools.cached_property
    def by_acct(self):
        """{account key: sorted slot keys (hex)}"""
        ak = self.st["acct_key"].tobytes()
        sk = self.st["slot_key"].tobytes().hex()
        out = {}
        for i in range(len(self.st)):
            out.setdefault(ak[32 * i:32 * i + 32], []).append(
                sk[64 * i:64 * i + 64])
        return out

    @functools.cached_property
    def lv_storage(self):
        return _branch_levels(self.by_acct.values())

    @functools.cached_property
    def lv_account(self):
        return _branch_levels([[k.hex() for k in self.akeys]])

    @property
    def lv_account_sub(self):  # shard mode splits at the top nibble
        return {d: v for d, v in self.lv_account.items() if d > 0}

    @functools.cached_property
    def account_proofs(self):
        """(targets, pyref node lists): ~8 present keys spread over the
        state, near misses of four of them, four unrelated absent keys."""
        present = set(self.akeys)
        tg = [self.akeys[i] for i in _spread(len(self.akeys), 8)]
        tg += [k for k in (_near_miss(k, present) for k in tg[:4]) if k]
        tg += [bind.keccak256(b"absent-acct" + bytes([i])) for i in range(4)]
        items = sorted(
            (pyref.nibbles_of(k), pyref.account_value(
                int(a["nonce"]), int.from_bytes(bytes(a["balance"]), "big"),
                bytes(r), bytes(a["code_hash"])))
            for k, a, r in zip(self.akeys, self.acct, self.sroots))
        proofs = []
        with pyref.accelerated(bind.keccak256):
            for t in tg:
                nodes = []
                pyref._collect_proof(items, 0, pyref.nibbles_of(t), True,
                                     nodes)
                proofs.append(nodes)
        return tg, proofs

    @functools.cached_property
    def storage_proofs(self):
        """(pairs, present flags, pyref (root, nodes)): ~8 present slots
        spread over the state, near-miss and unrelated absent slots, a
        storage-less account and an absent account."""
        st, by_acct = self.st, self.by_acct
        pairs = [(bytes(st[i]["acct_key"]), bytes(st[i]["slot_key"]))
                 for i in _spread(len(st), 8)]
        for a, s in pairs[:4]:
            nm = _near_miss(s, {bytes.fromhex(h) for h in by_acct[a]})
            if nm:
                pairs.append((a, nm))
        pairs += [(pairs[i][0], bind.keccak256(b"absent-slot" + bytes([i])))
                  for i in range(2)]
        bare = [k for k in self.akeys if k not in by_acct]
        if bare:
            pairs.append((bare[0], pairs[0][1]))
        pairs.append((bind.keccak256(b"absent-acct"), pairs[0][1]))
        sub = {k: (0, 0, b"", {}) for k in bare[:1]}
        for a in {a for a, _ in pairs if a in by_acct}:
            rows = st[(st["acct_key"] == np.frombuffer(a, np.uint8))
                      .all(axis=1)]
            sub[a] = (0, 0, b"", {
                bytes(r["slot_key"]): int.from_bytes(bytes(r["value"]), "big")
                for r in rows})
        here = [a in by_acct and s.hex() in by_acct[a] for a, s in pairs]
        want = []
        for a, s in pairs:
            with pyref.accelerated(bind.keccak256):
                want.append(pyref.storage_proof(sub, a, s))
        return pairs, here, want


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return Ref(name)


def _table(cfg_name, state, c):
    """The path each configuration exists to reach (the issue's table),
    asserted directly on the states wide enough to reach it."""
    if cfg_name == "base":
        assert c["class_levels"] == 0 and c["pipe2_levels"] == 0, c
    if cfg_name != "natural" and state not in WIDE:
        return
    if cfg_name == "cls":
        assert c["class_levels"] > 0 and c["fused_groups"] > 0, c
        assert c["pipe2_levels"] == 0, c
    elif cfg_name in ("cls+chunk", "natural"):
        assert c["class_levels"] > 0 and c["fused_groups"] > 0, c
        assert c["pipe2_levels"] > 0, c
    elif cfg_name == "split+chunk":
        assert c["class_levels"] > 0 and c["fused_groups"] == 0, c
        assert c["pipe2_levels"] > 0, c
    elif cfg_name == "chunk-only":
        assert c["class_levels"] == 0 and c["fused_groups"] == 0, c
        assert c["pipe2_levels"] > 0, c


@both
def test_roots(cfg, state):
    cfg_name, eng = cfg
    r = ref_of(state)
    eng.upload(r.acct, r.st)
    tag = f"{cfg_name} / {state}"
    ncalls = 3 if cfg_name == "cls+chunk" else 1  # same upload, no retries
    for call in range(ncalls):
        assert eng.root() == r.root, f"{tag}, call {call}"
    c = eng.path_counters()
    assert c == _expect([(r.lv_storage, True), (r.lv_account, True)],
                        cfg_name), tag
    _table(cfg_name, state, c)
    levels = eng.stats()["levels"]
    assert levels == len(r.lv_storage) + len(r.lv_account), tag
    if c["pipe2_levels"]:
        assert c["chunks"] > levels, (tag, c)
    else:
        assert c["chunks"] == levels, (tag, c)

    got = eng.storage_roots(len(r.acct))
    bad = np.nonzero((got != r.sroots).any(axis=1))[0]
    assert not len(bad), \
        f"{tag}: storage root of account {bytes(r.acct[bad[0]]['key']).hex()}"
    assert eng.path_counters() == _expect([(r.lv_storage, True)],
                                          cfg_name), tag

    refs, lens, roots, counts = eng.subtree_roots()
    assert eng.path_counters() == _expect(
        [(r.lv_storage, True), (r.lv_account_sub, True)], cfg_name), tag
    assert np.array_equal(lens, r.subtree[1]), tag
    assert np.array_equal(refs, r.subtree[0]), tag
    assert np.array_equal(roots, r.subtree[2]), tag
    assert eng.finish_top(refs, lens, roots, counts) == r.root, tag


@both
def test_updates(cfg, state):
    cfg_name, eng = cfg
    r = ref_of(state)
    eng.upload(r.acct, r.st)
    tag = f"{cfg_name} / {state}"
    root, rows = eng.root_with_updates()
    # rows are written through d_perm / urowidx; the fused kernel keeps
    # no meta to emit from, so it must be off here
    c = eng.path_counters()
    assert c == _expect([(r.lv_storage, False), (r.lv_account, False)],
                        cfg_name), tag
    assert c["fused_groups"] == 0
    want_root, want_rows = r.updates
    assert root == want_root == r.root, tag
    assert len(rows) == len(want_rows), (tag, len(rows), len(want_rows))
    ga = rows.view(np.uint8).reshape(len(rows), rows.itemsize)
    wa = want_rows.view(np.uint8).reshape(len(rows), rows.itemsize)
    bad = np.nonzero((ga != wa).any(axis=1))[0]
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{tag}: {len(bad)} rows differ; row {i}: "
                             f"engine={rows[i]} oracle={want_rows[i]}")


@both
def test_proofs(cfg, state):
    cfg_name, eng = cfg
    r = ref_of(state)
    eng.upload(r.acct, r.st)
    tag = f"{cfg_name} / {state}"
    present = set(r.akeys)
    targets, want_proofs = r.account_proofs
    proofs = eng.account_proof(targets)
    # proof rows are grabbed through cinv; the storage pass below the
    # account walk carries no targets and may still use the fused kernel
    assert eng.path_counters() == _expect(
        [(r.lv_storage, True), (r.lv_account, False)], cfg_name), tag
    for key, nodes, want in zip(targets, proofs, want_proofs):
        assert nodes == want, f"{tag}: account proof {key.hex()}"
        leaf = _replay(nodes, key, r.root)
        assert (leaf is not None) == (key in present), key.hex()

    if not len(r.st):
        with pytest.raises(RuntimeError):  # documented: needs storage
            eng.storage_proof([targets[0]], [targets[0]])
        return
    pairs, here_flags, want_sproofs = r.storage_proofs
    aks = [a for a, _ in pairs]
    sks = [s for _, s in pairs]
    roots, proofs = eng.storage_proof(aks, sks)
    assert eng.path_counters() == _expect([(r.lv_storage, False)],
                                          cfg_name), tag
    for a, s, here, root, nodes, (wroot, wnodes) in zip(
            aks, sks, here_flags, roots, proofs, want_sproofs):
        assert root == wroot, f"{tag}: storage root {a.hex()}"
        assert nodes == wnodes, f"{tag}: storage proof {a.hex()}/{s.hex()}"
        assert nodes or not here
        if nodes:
            assert (_replay(nodes, s, root) is not None) == here, s.hex()
