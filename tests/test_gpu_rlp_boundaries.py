"""Leaf and branch RLP at the length boundaries where the kernels change
path: the storage-leaf register/LDS switch at D = 13/14 crossed with every
value length, account leaves around the 136-byte keccak block boundary,
and branch nodes of exactly chosen RLP lengths (inline children, header
growth, 1/2/3/4 keccak blocks). Default size gates; the same corpora run
under the lowered gates in test_gpu_pipeline_gates.py.

The corpora come from tests/rlp_corpus.py; tests/test_rlp_corpus_cpu.py
proves on the CPU that each target length is really present. Everything
is bit-exact against the C oracle, and against pyref where named."""
import functools

import numpy as np
import pytest

from oracle import bind, pyref
from tests import rlp_corpus as rc
from tests.util import to_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


def _check_roots(eng, acct, st, tag):
    want = bind.state_root(acct, st)
    eng.upload(acct, st)
    assert eng.root() == want, tag
    refs, lens, roots, counts = eng.subtree_roots()
    o = bind.subtree_roots(acct, st)
    assert np.array_equal(lens, o[1]), tag
    assert np.array_equal(refs, o[0]), tag
    assert np.array_equal(roots, o[2]), tag
    assert eng.finish_top(refs, lens, roots, counts) == want, tag


@functools.lru_cache(maxsize=None)
def _leaf_grid():
    accounts, labels = rc.storage_leaf_grid()
    acct, st = to_arrays(dict(accounts))
    return dict(accounts), labels, acct, st, bind.storage_roots(acct, st)


def test_storage_leaf_grid(eng):
    accounts, labels, acct, st, want = _leaf_grid()
    eng.upload(acct, st)
    got = eng.storage_roots(len(acct))
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        D, L, cls, v = labels[bytes(acct[bad[0]]["key"])]
        raise AssertionError(
            f"{len(bad)} storage roots differ; first: D={D} L={L} "
            f"class={cls} value={v:#x} engine={bytes(got[bad[0]]).hex()} "
            f"oracle={bytes(want[bad[0]]).hex()}")
    # the rows around the leaf kernel's path switch and at both ends of
    # the depth range, against the independent pure-Python reference
    for i, a in enumerate(acct):
        key = bytes(a["key"])
        if labels[key][0] in (-1, 0, 12, 13, 14, 62, 63):
            assert bytes(got[i]) == pyref.storage_root(accounts[key][3]), \
                labels[key]
    assert eng.root() == bind.state_root(acct, st)


@pytest.mark.parametrize("nonce_len", range(9))
def test_account_leaf_grid(eng, nonce_len):
    accounts, labels = rc.account_leaf_grid(nonce_len)
    acct, st = to_arrays(dict(accounts))
    _check_roots(eng, acct, st, f"nonce byte length {nonce_len}")
    if nonce_len in (0, 8):  # pure-Python cross-check at the two extremes
        assert eng.root() == pyref.state_root(dict(accounts))


@pytest.mark.parametrize("total", [135, 136, 137, 138])
def test_single_account_leaf_at_block_boundary(eng, total):
    accounts = dict(rc.single_account_states())[total]
    acct, st = to_arrays(dict(accounts))
    _check_roots(eng, acct, st, f"single account, leaf RLP {total} B")
    assert eng.root() == pyref.state_root(dict(accounts))


def test_branch_length_state(eng):
    accounts, labels = rc.branch_length_state()
    acct, st = to_arrays(dict(accounts))
    want = bind.storage_roots(acct, st)
    eng.upload(acct, st)
    got = eng.storage_roots(len(acct))
    bad = sorted({labels[bytes(acct[i]["key"])]
                  for i in np.nonzero((got != want).any(axis=1))[0]})
    assert not bad, f"storage roots differ for branch-length tries {bad}"
    tries = rc.branch_length_tries()
    ref = {name: pyref.storage_root(slots) for name, slots in tries.items()}
    for i, a in enumerate(acct):
        assert bytes(got[i]) == ref[labels[bytes(a["key"])]]
    _check_roots(eng, acct, st, "branch-length state")
