"""The CPU side of the plain-state upload, without a GPU:

  - tests/plain_model.py (the reference the GPU tests compare with) turns
    the three genesis fixtures' plain addresses and slots, shuffled, into
    rows whose oracle root is the consensus root;
  - its expected counters are what they should be on hand-checkable inputs;
  - the plain row layouts are 96 and 84 bytes, and the numpy and torch
    generators of reth_amd.plain agree;
  - reth_amd/csrc/radix.h is checked by a plain host executable
    (tests/hashsort_main.cpp) built with the address and
    undefined-behaviour sanitizers. Nothing is loaded into Python.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import bind
from reth_amd import plain
from reth_amd.engine import PLAIN_ACCOUNT_DTYPE, PLAIN_STORAGE_DTYPE
from tests import plain_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "reth_amd", "csrc")


def test_plain_dtype_sizes():
    assert PLAIN_ACCOUNT_DTYPE.itemsize == 96
    assert PLAIN_STORAGE_DTYPE.itemsize == 84
    assert PLAIN_ACCOUNT_DTYPE.fields["nonce"][1] == 24
    assert PLAIN_ACCOUNT_DTYPE.fields["balance"][1] == 32
    assert PLAIN_STORAGE_DTYPE.fields["value"][1] == 52


@pytest.mark.parametrize("name", ["mainnet", "sepolia", "holesky"])
def test_model_reaches_consensus_root_from_plain_genesis(name):
    acct, st, root = pm.genesis_plain(name, seed=1)
    m = pm.Model(acct, st)
    assert len(m.acct) == len(acct) and len(m.st) == len(st)
    assert bind.state_root(m.acct, m.st) == root
    # sorted, strictly
    k = [bytes(x) for x in m.acct["key"]]
    assert all(a < b for a, b in zip(k, k[1:]))
    sk = [bytes(a) + bytes(s) for a, s in zip(m.st["acct_key"], m.st["slot_key"])]
    assert all(a < b for a, b in zip(sk, sk[1:]))


def test_model_is_order_independent():
    acct, st = plain.gen_plain_numpy(300, 3)
    m0 = pm.Model(acct, st)
    m1 = pm.Model(*pm.shuffled(acct, st, 7))
    assert m0.acct.tobytes() == m1.acct.tobytes()
    assert m0.st.tobytes() == m1.st.tobytes()
    assert m0.counters() == m1.counters()


def test_model_counters_on_small_inputs():
    # empty state: nothing hashed, no sort at all
    a0, s0 = plain.gen_plain_numpy(0, 0)
    assert pm.Model(a0, s0).counters() == {
        "keccak_f": 0, "passes": 0, "skipped": 0, "tie_rows": 0,
        "tie_runs": 0, "addr_reused": 0}
    # one account, one slot: every digit is shared by the only key
    a1, s1 = plain.gen_plain_numpy(1, 1)
    c = pm.Model(a1, s1).counters()
    assert (c["keccak_f"], c["passes"], c["skipped"]) == (3, 0, 16)
    # one account, 300 slots: rank 0, so only the four slot-prefix passes
    a, s = plain.gen_plain_numpy(1, 300)
    m = pm.Model(a, s)
    assert m.passes() == ((0, 8), (4, 4))
    # K = 0 wipes the whole prefix: one run holds every storage row
    c = m.counters(key_bits=0)
    assert (c["passes"], c["tie_rows"], c["tie_runs"]) == (0, 300, 1)
    # K = 4 keeps one nibble: at most 16 distinct keys, one pass
    c = m.counters(key_bits=4)
    assert c["passes"] == 1 and c["tie_runs"] <= 16 and c["tie_rows"] >= 300 - 16
    # 257 accounts need two rank bytes
    a, s = plain.gen_plain_numpy(257, 2)
    assert pm.Model(a, s).passes()[1] == (6, 2)


def test_numpy_and_torch_generators_agree():
    import torch
    counts = np.array([0, 1, 5, 0, 64, 3, 2], dtype=np.int64)
    a_np, s_np = plain.gen_plain_numpy(7, counts, first=11)
    a_t, s_t = plain.gen_plain_torch(7, torch.from_numpy(counts), device="cpu",
                                     first=11)
    a2, s2 = plain.tensors_to_np_plain(a_t, s_t)
    assert a_np.tobytes() == a2.tobytes()
    assert s_np.tobytes() == s2.tobytes()
    a_np, s_np = plain.gen_plain_numpy(100, 4)
    a_t, s_t = plain.gen_plain_torch(100, 4, device="cpu")
    a2, s2 = plain.tensors_to_np_plain(a_t, s_t)
    assert a_np.tobytes() == a2.tobytes() and s_np.tobytes() == s2.tobytes()
    assert len(set(bytes(x) for x in a_np["address"])) == 100
    assert (s_np["value"].reshape(-1, 32).max(axis=1) > 0).all()


def test_radix_header_matches_byte_loops(tmp_path):
    exe = str(tmp_path / "hashsort_check")
    r = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(HERE, "hashsort_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checked, failed = (int(x) for x in r.stdout.split()[1::2])
    # keys: 2000 hashes x 13 gates x (2 keys + 8 digits); compare: 200k
    # pairs both ways; passes: 16 sizes x 3 key spreads x 4 checks
    assert failed == 0 and checked == 2000 * 13 * 10 + 400_000 + 16 * 3 * 4, \
        r.stdout
