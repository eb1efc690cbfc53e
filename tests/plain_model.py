"""CPU reference of the plain-state upload (include/sre.h
sre_upload_plain_state): what the engine must make resident from plain
rows, and what its hash-and-sort counters must read.

Keys come from the oracle's keccak (bind.keccak256_batch), the order from
np.lexsort over the full hashed keys. The expected counters come from the
same data: the radix passes from the digits the reference 64-bit sort keys
actually share, the tie rows and runs from equal sort keys under a given
SRE_HS_KEY_BITS. Nothing here looks at the engine.
"""
import gzip
import json
import os

import numpy as np

from oracle import bind, pyref
from reth_amd.engine import PLAIN_ACCOUNT_DTYPE, PLAIN_STORAGE_DTYPE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _keccak_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if len(rows) == 0:
        return np.zeros((0, 32), dtype=np.uint8)
    return bind.keccak256_batch(rows)


def _be_cols(keys):
    """(n,32) u8 -> four u64 columns, most significant first."""
    return [keys[:, 8 * k:8 * (k + 1)].copy().view(">u8").ravel().astype(np.uint64)
            for k in range(4)]


def _keep_top(prefix, width, key_bits):
    """radix.h hs_keep_top on a u64 array."""
    if key_bits is None or key_bits >= width:
        return prefix
    if key_bits == 0:
        return np.zeros_like(prefix)
    mask = ((1 << width) - 1) & ~((1 << (width - key_bits)) - 1)
    return prefix & np.uint64(mask)


class Model:
    """The expected resident arrays and sort keys of one plain state."""

    def __init__(self, accounts, storage):
        assert accounts.dtype == PLAIN_ACCOUNT_DTYPE
        assert storage.dtype == PLAIN_STORAGE_DTYPE
        na, ns = len(accounts), len(storage)
        hk = _keccak_rows(accounts["address"].reshape(na, 20))
        cols = _be_cols(hk)
        order = np.lexsort(tuple(reversed(cols)))
        self.acct = np.zeros(na, dtype=bind.ACCOUNT_DTYPE)
        self.acct["key"] = hk[order]
        self.acct["nonce"] = accounts["nonce"][order]
        self.acct["balance"] = accounts["balance"][order]
        self.acct["code_hash"] = accounts["code_hash"][order]
        self._acct_prefix = cols[0]
        self.order = order      # acct[i] comes from accounts[order[i]]

        ha = _keccak_rows(storage["address"].reshape(ns, 20))
        hs = _keccak_rows(storage["slot"].reshape(ns, 32))
        rank_of = {k.tobytes(): i for i, k in enumerate(self.acct["key"])}
        assert len(rank_of) == na, "duplicate address in the model's input"
        rank = np.array([rank_of[h.tobytes()] for h in ha], dtype=np.uint64)
        scols = _be_cols(hs)
        sorder = np.lexsort(tuple(reversed(scols)) + (rank,))
        self.st = np.zeros(ns, dtype=bind.STORAGE_DTYPE)
        self.st["acct_key"] = ha[sorder]
        self.st["slot_key"] = hs[sorder]
        self.st["value"] = storage["value"][sorder]
        self._rank = rank
        self.sorder = sorder    # st[i] comes from storage[sorder[i]]
        self._slot_prefix = scols[0] >> np.uint64(32)

    def sort_keys(self, key_bits=None):
        """The 64-bit radix keys (radix.h hs_account_key / hs_storage_key)."""
        a = _keep_top(self._acct_prefix, 64, key_bits)
        s = (self._rank << np.uint64(32)) | _keep_top(self._slot_prefix, 32,
                                                      key_bits)
        return a, s

    @staticmethod
    def _passes(keys):
        """(executed, skipped): a pass runs iff its digit is not shared."""
        if len(keys) == 0:
            return 0, 0
        ran = sum(1 for p in range(8)
                  if len(np.unique((keys >> np.uint64(8 * p)) & np.uint64(255))) > 1)
        return ran, 8 - ran

    @staticmethod
    def _ties(keys):
        """(rows in runs, runs) of equal sort keys, runs of length >= 2."""
        if len(keys) == 0:
            return 0, 0
        _, counts = np.unique(keys, return_counts=True)
        runs = counts[counts >= 2]
        return int(runs.sum()), int(len(runs))

    def passes(self, key_bits=None):
        """((account executed, skipped), (storage executed, skipped))"""
        a, s = self.sort_keys(key_bits)
        return self._passes(a), self._passes(s)

    def counters(self, key_bits=None):
        """engine.hash_sort_counters() of a successful upload."""
        a, s = self.sort_keys(key_bits)
        (ar, ask), (sr, ssk) = self._passes(a), self._passes(s)
        (atr, atn), (str_, stn) = self._ties(a), self._ties(s)
        return {"keccak_f": len(a) + 2 * len(s), "passes": ar + sr,
                "skipped": ask + ssk, "tie_rows": atr + str_,
                "tie_runs": atn + stn, "addr_reused": 0}


def shuffled(accounts, storage, seed):
    rng = np.random.default_rng(seed)
    return (accounts[rng.permutation(len(accounts))],
            storage[rng.permutation(len(storage))])


def genesis_plain(name, seed=0):
    """A genesis fixture as shuffled plain rows -> (accounts, storage,
    consensus root bytes)."""
    d = json.load(gzip.open(os.path.join(GOLDEN, f"genesis_{name}.json.gz"), "rt"))
    rows, strows = [], []
    for a, nonce, bal, code, storage in d["accounts"]:
        addr = bytes.fromhex(a)
        assert len(addr) == 20
        ch = bind.keccak256(bytes.fromhex(code)) if code else pyref.KECCAK_EMPTY
        rows.append((addr, nonce, int(bal, 16), ch))
        for s, v in storage.items():
            strows.append((addr, bytes.fromhex(s), int(v, 16)))
    acct = np.zeros(len(rows), dtype=PLAIN_ACCOUNT_DTYPE)
    for i, (addr, nonce, bal, ch) in enumerate(rows):
        acct[i]["address"] = np.frombuffer(addr, np.uint8)
        acct[i]["nonce"] = nonce
        acct[i]["balance"] = np.frombuffer(bal.to_bytes(32, "big"), np.uint8)
        acct[i]["code_hash"] = np.frombuffer(ch, np.uint8)
    st = np.zeros(len(strows), dtype=PLAIN_STORAGE_DTYPE)
    for i, (addr, slot, v) in enumerate(strows):
        st[i]["address"] = np.frombuffer(addr, np.uint8)
        st[i]["slot"] = np.frombuffer(slot.rjust(32, b"\0"), np.uint8)
        st[i]["value"] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)
    acct, st = shuffled(acct, st, seed)
    root = d["state_root"]
    return acct, st, bytes.fromhex(root[2:] if root.startswith("0x") else root)
