"""ctypes binding over the C-ABI of the MI355X state-root engine (libsre.so).

Product path: GPU-only. Raises RuntimeError at construction when no HIP
device / extension is present — there is no CPU fallback (the CPU oracle
under oracle/ is test infrastructure and must never be imported here).

Mirrors the reference surface it replaces (see include/sre.h):
  StateRootEngine.root()           ~ StateRoot::root() /
                                     StateRootProvider::state_root
                                     (/root/reference/crates/storage/storage-api/src/trie.rs:13-41)
  StateRootEngine.storage_roots()  ~ StorageRootProvider::storage_root (:45-58)
  subtree_roots()/finish_top()     ~ the multi-GPU decomposition of
                                     StateRoot::calculate (crates/trie/trie/src/trie.rs:171)
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libsre.so")
SRC = os.path.join(HERE, "csrc", "sre.hip")

ACCOUNT_DTYPE = np.dtype([
    ("key", np.uint8, 32),
    ("nonce", np.uint64),
    ("balance", np.uint8, 32),
    ("code_hash", np.uint8, 32),
])
STORAGE_DTYPE = np.dtype([
    ("acct_key", np.uint8, 32),
    ("slot_key", np.uint8, 32),
    ("value", np.uint8, 32),
])

# sre_account_delta (include/sre.h): one overlay-delta account row
DELTA_DTYPE = np.dtype([
    ("key", np.uint8, 32),
    ("nonce", np.uint64),
    ("balance", np.uint8, 32),
    ("code_hash", np.uint8, 32),
    ("deleted", np.uint8),
    ("pad", np.uint8, 7),
])
assert DELTA_DTYPE.itemsize == 112

# sre_update_row (include/sre.h): one stored BranchNodeCompact + its path
UPDATE_DTYPE = np.dtype([
    ("acct_key", np.uint8, 32),
    ("kind", np.uint8),
    ("path_len", np.uint8),
    ("path", np.uint8, 32),
    ("num_hashes", np.uint8),
    ("root_hash_set", np.uint8),
    ("state_mask", "<u2"),
    ("tree_mask", "<u2"),
    ("hash_mask", "<u2"),
    ("root_hash", np.uint8, 32),
    ("hashes", np.uint8, (16, 32)),
    # incremental net-diff marker: 0 upsert, 1 removed path,
    # 2 whole-storage-trie deletion (destroyed account) — include/sre.h
    ("removed", np.uint8),
    ("pad", np.uint8, 5),
])
assert UPDATE_DTYPE.itemsize == 624

# sre_plain_account / sre_plain_storage (include/sre.h): unhashed rows
PLAIN_ACCOUNT_DTYPE = np.dtype([
    ("address", np.uint8, 20),
    ("pad", np.uint8, 4),
    ("nonce", np.uint64),
    ("balance", np.uint8, 32),
    ("code_hash", np.uint8, 32),
])
assert PLAIN_ACCOUNT_DTYPE.itemsize == 96
PLAIN_STORAGE_DTYPE = np.dtype([
    ("address", np.uint8, 20),
    ("slot", np.uint8, 32),
    ("value", np.uint8, 32),
])
assert PLAIN_STORAGE_DTYPE.itemsize == 84


class SreStats(ctypes.Structure):
    _fields_ = [
        ("total_ms", ctypes.c_double),
        ("leaf_hash_ms", ctypes.c_double),
        ("leaf_count", ctypes.c_uint64),
        ("leaf_blocks", ctypes.c_uint64),
        ("branch_hash_ms", ctypes.c_double),
        ("branch_count", ctypes.c_uint64),
        ("branch_blocks", ctypes.c_uint64),
        ("sort_ms", ctypes.c_double),
        ("levels", ctypes.c_uint64),
    ]


def build(verbose=False):
    """Compile libsre.so for gfx950 (in-tree; the .so travels with the repo)."""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared",
           "-fPIC", SRC, "-o", LIB]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed:\n{r.stdout}\n{r.stderr}")
    if verbose:
        print(f"built {LIB}")


_P, _U64, _U32, _INT = (ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                        ctypes.c_int)
_DELTA = [_P, _P, _U64, _P, _U64]  # ctx, account rows, n, storage rows, n

# Every entry point of include/sre.h, grouped by (restype, argtypes); lib()
# applies them, so no call site converts an argument by hand. Scalars map by
# C type (uint64_t, uint32_t, int); every pointer or array parameter is
# c_void_p, which takes numpy pointers, None, ctypes arrays and byref
# objects. tests/test_abi_cpu.py checks the table against the header.
_SIGNATURES = (
    (_P, [_INT], "sre_create"),
    (None, [_P], "sre_destroy"),
    (ctypes.c_char_p, [_P], "sre_last_error"),
    (ctypes.c_int64, [_P], "sre_updates_count"),
    (_INT, [_P, _INT], "sre_set_revert_capture"),
    (_INT, [_P, _P],  # ctx, one output
     "sre_root sre_root_with_updates sre_root_retaining "
     "sre_root_retaining_with_updates sre_unwind sre_unwind_with_updates "
     "sre_get_stats sre_get_path_counters sre_get_incremental_counters "
     "sre_get_hash_sort_counters sre_get_revert_counters"),
    (_INT, [_P, _P, _P], "sre_resident_counts sre_revert_counts"),
    (_INT, [_P, _P, _U64],  # ctx, rows, count
     "sre_upload_accounts sre_upload_storage sre_set_accounts_device "
     "sre_set_storage_device sre_download_accounts sre_download_storage "
     "sre_updates_get sre_storage_roots"),
    (_INT, _DELTA, "sre_upload_plain_state sre_set_plain_state_device "
                   "sre_apply_delta sre_revert_get"),
    (_INT, _DELTA + [_P],
     "sre_incremental_root sre_incremental_root_with_updates"),
    (_INT, [_P, _P, _U64, _P, _U64, _P, _U64, _P],
     "sre_root_from_nodes sre_account_proof"),
    (_INT, [_P, _P, _P, _U64, _P, _P, _U64, _P, _U64, _P], "sre_storage_proof"),
    (_INT, [_P, _P, _U64, _U32, _U64, _P],
     "sre_keccak_batch_device sre_keccak_long_device"),
    (_INT, [_P] * 5, "sre_subtree_roots"),
    (_INT, [_P] * 6, "sre_finish_top"),
)
ABI = {name: (restype, argtypes) for restype, argtypes, names in _SIGNATURES
       for name in names.split()}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError(
                f"{LIB} missing — run __graft_entry__.build() / reth_amd.engine.build()")
        _lib = ctypes.CDLL(LIB)
        for name, (restype, argtypes) in ABI.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return _lib


def _np_ptr(arr):
    if len(arr) == 0:
        return None
    return arr.ctypes.data_as(ctypes.c_void_p)


class StateRootEngine:
    def __init__(self, device=0):
        self._lib = lib()
        self._ctx = self._lib.sre_create(device)
        if not self._ctx:
            raise RuntimeError("sre_create failed (GPU required, no fallback): "
                               + self._lib.sre_last_error(None).decode())
        self._keep = []  # borrowed device tensors kept alive

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.sre_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.sre_last_error(self._ctx).decode())

    def _root(self, fn, *args):
        """Call a root-type entry point: its arguments, then the 32-byte
        output root, which is returned."""
        out = (ctypes.c_uint8 * 32)()
        self._check(fn(self._ctx, *args, out))
        return bytes(out)

    # ---- input upload ----
    def upload(self, accounts: np.ndarray, storage: np.ndarray):
        assert accounts.dtype == ACCOUNT_DTYPE and storage.dtype == STORAGE_DTYPE
        self._check(self._lib.sre_upload_accounts(
            self._ctx, _np_ptr(accounts), len(accounts)))
        self._check(self._lib.sre_upload_storage(
            self._ctx, _np_ptr(storage), len(storage)))

    def set_device_tensors(self, acct_u8, st_u8):
        """Borrow torch GPU tensors: acct (na,104) uint8, st (ns,96) uint8,
        contiguous, laid out as sre_account_entry / sre_storage_entry."""
        assert acct_u8.dtype.itemsize == 1 and acct_u8.is_contiguous()
        assert st_u8.dtype.itemsize == 1 and st_u8.is_contiguous()
        assert acct_u8.shape[1] == 104 and st_u8.shape[1] == 96
        self._keep = [acct_u8, st_u8]
        self._check(self._lib.sre_set_accounts_device(
            self._ctx, acct_u8.data_ptr(), acct_u8.shape[0]))
        self._check(self._lib.sre_set_storage_device(
            self._ctx, st_u8.data_ptr(), st_u8.shape[0]))

    def upload_plain(self, accounts: np.ndarray, storage: np.ndarray):
        """Replace the resident state by the hashed, sorted form of plain
        rows (PLAIN_ACCOUNT_DTYPE / PLAIN_STORAGE_DTYPE, any order): the
        engine hashes addresses and slots and sorts on the device
        (include/sre.h sre_upload_plain_state)."""
        assert accounts.dtype == PLAIN_ACCOUNT_DTYPE
        assert storage.dtype == PLAIN_STORAGE_DTYPE
        accounts = np.ascontiguousarray(accounts)
        storage = np.ascontiguousarray(storage)
        self._check(self._lib.sre_upload_plain_state(
            self._ctx, _np_ptr(accounts), len(accounts), _np_ptr(storage),
            len(storage)))
        self._keep = []  # the new state is engine-owned

    def set_plain_device_tensors(self, acct_u8, st_u8):
        """upload_plain from torch GPU tensors: acct (na,96) uint8, st
        (ns,84) uint8, contiguous, laid out as sre_plain_account /
        sre_plain_storage. The engine reads them during the call only and
        keeps no reference. Its kernels run on the engine's own stream:
        drain torch's first, as in _keccak_device."""
        import torch
        assert acct_u8.dtype.itemsize == 1 and acct_u8.is_contiguous()
        assert st_u8.dtype.itemsize == 1 and st_u8.is_contiguous()
        assert acct_u8.shape[1] == 96 and st_u8.shape[1] == 84
        if acct_u8.is_cuda:
            torch.cuda.synchronize(acct_u8.device)
        na, ns = acct_u8.shape[0], st_u8.shape[0]
        self._check(self._lib.sre_set_plain_state_device(
            self._ctx, acct_u8.data_ptr() if na else None, na,
            st_u8.data_ptr() if ns else None, ns))
        self._keep = []

    def _counts(self, fn):
        na, ns = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(fn(self._ctx, ctypes.byref(na), ctypes.byref(ns)))
        return na.value, ns.value

    def resident_counts(self):
        return self._counts(self._lib.sre_resident_counts)

    def download(self):
        """The resident state as (ACCOUNT_DTYPE array, STORAGE_DTYPE array):
        the sorted hashed rows, whatever made them resident."""
        na, ns = self.resident_counts()
        acct = np.zeros(na, dtype=ACCOUNT_DTYPE)
        st = np.zeros(ns, dtype=STORAGE_DTYPE)
        self._check(self._lib.sre_download_accounts(
            self._ctx, _np_ptr(acct), na))
        self._check(self._lib.sre_download_storage(self._ctx, _np_ptr(st), ns))
        return acct, st

    def hash_sort_counters(self) -> dict:
        """What the last plain upload did (include/sre.h
        sre_get_hash_sort_counters)."""
        out = (ctypes.c_uint64 * 6)()
        self._check(self._lib.sre_get_hash_sort_counters(self._ctx, out))
        return {"keccak_f": out[0], "passes": out[1], "skipped": out[2],
                "tie_rows": out[3], "tie_runs": out[4], "addr_reused": out[5]}

    def release_borrowed(self):
        """Drop the references keeping borrowed device tensors alive
        (set_device_tensors). Precondition: the engine no longer reads
        them — i.e. the resident state has been replaced by engine-owned
        arrays (apply_delta / incremental_root adopt merged copies first),
        or new tensors were set. After this the caller may free the
        tensors (torch.cuda.empty_cache())."""
        self._keep = []

    def apply_delta(self, acct_delta: np.ndarray, st_delta: np.ndarray):
        """Apply a HashedPostState overlay delta to the resident state
        (post-state wins, zero value deletes a slot, deleted accounts wipe
        their storage). A following root() computes the post-delta root —
        the incremental-root entry (BASELINE configs[4])."""
        assert acct_delta.dtype == DELTA_DTYPE
        assert st_delta.dtype == STORAGE_DTYPE
        self._check(self._lib.sre_apply_delta(
            self._ctx, _np_ptr(acct_delta), len(acct_delta), _np_ptr(st_delta),
            len(st_delta)))

    # ---- compute ----
    def root_retaining(self) -> bytes:
        """Full root that also retains cell-top trie records and every
        account's storage root, so following incremental_root() calls
        recompute only what a delta touches. See include/sre.h
        sre_root_retaining."""
        return self._root(self._lib.sre_root_retaining)

    def incremental_root(self, acct_delta: np.ndarray,
                         st_delta: np.ndarray = None) -> bytes:
        """Apply a HashedPostState overlay delta (accounts + storage) and
        recompute the root along dirty paths only (requires a prior
        root_retaining): untouched accounts keep their retained storage
        roots, touched storage tries are rebuilt from their merged
        segments, and only delta-touched account-trie cells rehash. The
        resident state becomes the merged result and retention is
        refreshed, so deltas chain."""
        assert acct_delta.dtype == DELTA_DTYPE
        if st_delta is None:
            st_delta = np.zeros(0, dtype=STORAGE_DTYPE)
        assert st_delta.dtype == STORAGE_DTYPE
        return self._root(self._lib.sre_incremental_root,
                          _np_ptr(acct_delta), len(acct_delta),
                          _np_ptr(st_delta), len(st_delta))

    def root(self) -> bytes:
        return self._root(self._lib.sre_root)

    def _fetch_updates(self):
        n = self._lib.sre_updates_count(self._ctx)
        rows = np.zeros(n, dtype=UPDATE_DTYPE)
        if n:
            self._check(self._lib.sre_updates_get(self._ctx, _np_ptr(rows), n))
        return rows

    def root_retaining_with_updates(self):
        """Full root + full TrieUpdates row set, AND arms both the cell-top
        retention and the stored-row snapshot so following
        incremental_root_with_updates calls emit net row diffs
        (include/sre.h sre_root_retaining_with_updates)."""
        root = self._root(self._lib.sre_root_retaining_with_updates)
        return root, self._fetch_updates()

    def incremental_root_with_updates(self, acct_delta: np.ndarray,
                                      st_delta: np.ndarray = None):
        """Dirty-path incremental root + the NET TrieUpdates diff vs the
        pre-delta trie: upserts (removed=0), removals (removed=1,
        walker.rs:363-369 removed_nodes semantics) and destroyed-account
        whole-storage-trie markers (removed=2, updates.rs:154-157).
        Applying the diff to the pre-delta row set reproduces the full
        row set of the post-delta state. Requires a prior
        root_retaining_with_updates; deltas chain."""
        assert acct_delta.dtype == DELTA_DTYPE
        if st_delta is None:
            st_delta = np.zeros(0, dtype=STORAGE_DTYPE)
        assert st_delta.dtype == STORAGE_DTYPE
        root = self._root(self._lib.sre_incremental_root_with_updates,
                          _np_ptr(acct_delta), len(acct_delta),
                          _np_ptr(st_delta), len(st_delta))
        return root, self._fetch_updates()

    def root_from_nodes(self, rows: np.ndarray, acct_delta: np.ndarray = None,
                        st_delta: np.ndarray = None) -> bytes:
        """state_root_from_nodes / TrieInput equivalent: root of
        (resident state + delta) with `rows` (UPDATE_DTYPE, e.g. from
        root_with_updates) seeding untouched accounts' storage roots so
        their tries are not recomputed (include/sre.h
        sre_root_from_nodes). Replaces the resident state with the
        merged result."""
        assert rows.dtype == UPDATE_DTYPE
        if acct_delta is None:
            acct_delta = np.zeros(0, dtype=DELTA_DTYPE)
        if st_delta is None:
            st_delta = np.zeros(0, dtype=STORAGE_DTYPE)
        assert acct_delta.dtype == DELTA_DTYPE
        assert st_delta.dtype == STORAGE_DTYPE
        return self._root(self._lib.sre_root_from_nodes,
                          _np_ptr(rows), len(rows),
                          _np_ptr(acct_delta), len(acct_delta),
                          _np_ptr(st_delta), len(st_delta))

    def root_with_updates(self):
        """State root + TrieUpdates rows (UPDATE_DTYPE), sorted like reth's
        TrieUpdates::into_sorted. Surface of
        StateRootProvider::state_root_with_updates."""
        root = self._root(self._lib.sre_root_with_updates)
        return root, self._fetch_updates()

    def account_proof(self, targets, cap_nodes=None, cap_lens=None) -> list:
        """Account multiproof: per target, the proof node RLPs root-first
        (Proof::multiproof account surface, include/sre.h
        sre_account_proof). Present keys get the path to their leaf;
        absent keys get the exclusion proof ending at the divergence.
        targets: list of 32-byte hashed keys. cap_nodes / cap_lens
        override the output capacities (bytes / entries) handed to the
        engine; the defaults hold any proof."""
        return self._proofs(self._lib.sre_account_proof, [targets],
                            cap_nodes, cap_lens)

    def storage_proof(self, acct_keys, slot_keys, cap_nodes=None,
                      cap_lens=None):
        """Storage multiproof for (account, slot) pairs. The slot may be
        absent (exclusion proof); an absent or storage-less account
        yields (EMPTY_ROOT_HASH, []) = StorageMultiProof::empty().
        Returns (roots, proofs) — per target the account's storage root
        and the root-first node-RLP list of its storage trie. cap_nodes /
        cap_lens as in account_proof."""
        assert len(slot_keys) == len(acct_keys)
        roots = np.zeros((len(acct_keys), 32), dtype=np.uint8)
        proofs = self._proofs(self._lib.sre_storage_proof,
                              [acct_keys, slot_keys], cap_nodes, cap_lens,
                              [roots])
        return [bytes(r) for r in roots], proofs

    def _proofs(self, fn, key_lists, cap_nodes, cap_lens, extra_out=()):
        """Call a proof entry point (include/sre.h): its 32-byte key lists,
        the target count, extra_out, then the node / length / count
        outputs: counts[t] nodes per target, their byte lengths in lens,
        their bytes back to back in nodes. Returns per-target node lists."""
        n = len(key_lists[0])
        keys = [np.ascontiguousarray(np.frombuffer(
            b"".join(k), dtype=np.uint8).reshape(n, 32)) for k in key_lists]
        if cap_nodes is None:
            cap_nodes = n * 130 * 560 + 4096
        if cap_lens is None:
            cap_lens = n * 132
        nodes = np.zeros(cap_nodes, dtype=np.uint8)
        lens = np.zeros(cap_lens, dtype=np.uint32)
        counts = np.zeros(n, dtype=np.uint32)
        self._check(fn(
            self._ctx, *[_np_ptr(k) for k in keys], n,
            *[_np_ptr(o) for o in extra_out], _np_ptr(nodes), cap_nodes,
            _np_ptr(lens), cap_lens, _np_ptr(counts)))
        out, off, li = [], 0, 0
        for cnt in counts:
            tl = []
            for ln in lens[li:li + int(cnt)]:
                tl.append(nodes[off:off + int(ln)].tobytes())
                off += int(ln)
            li += int(cnt)
            out.append(tl)
        return out

    def storage_roots(self, n) -> np.ndarray:
        out = np.empty((n, 32), dtype=np.uint8)
        self._check(self._lib.sre_storage_roots(self._ctx, _np_ptr(out), n))
        return out

    def subtree_roots(self):
        refs = np.zeros((16, 33), dtype=np.uint8)
        lens = np.zeros(16, dtype=np.uint8)
        roots = np.zeros((16, 32), dtype=np.uint8)
        counts = np.zeros(16, dtype=np.uint64)
        self._check(self._lib.sre_subtree_roots(
            self._ctx, _np_ptr(refs), _np_ptr(lens), _np_ptr(roots),
            _np_ptr(counts)))
        return refs, lens, roots, counts

    def finish_top(self, refs, lens, roots, counts) -> bytes:
        return self._root(
            self._lib.sre_finish_top,
            _np_ptr(np.ascontiguousarray(refs, dtype=np.uint8)),
            _np_ptr(np.ascontiguousarray(lens, dtype=np.uint8)),
            _np_ptr(np.ascontiguousarray(roots, dtype=np.uint8)),
            _np_ptr(np.ascontiguousarray(counts, dtype=np.uint64)))

    def keccak_batch_device(self, in_tensor, msg_len, out_tensor):
        """Hash n messages of msg_len bytes at a fixed stride (device memory).
        in_tensor: (n, stride) uint8 cuda tensor; out_tensor: (n, 32) uint8.

        The kernel runs on the engine's own HIP stream: drain torch's stream
        first so pending writes to in_tensor are visible (the engine
        synchronizes its stream before returning, so later torch ops are
        safe the other way around)."""
        return self._keccak_device(self._lib.sre_keccak_batch_device,
                                   in_tensor, msg_len, out_tensor)

    def keccak_long_device(self, in_tensor, msg_len, out_tensor):
        """keccak_batch_device without the one-block limit: msg_len may be
        anything up to the row stride (multi-block messages)."""
        return self._keccak_device(self._lib.sre_keccak_long_device,
                                   in_tensor, msg_len, out_tensor)

    def _keccak_device(self, fn, in_tensor, msg_len, out_tensor):
        import torch
        if in_tensor.is_cuda:
            torch.cuda.synchronize(in_tensor.device)
        n, stride = in_tensor.shape
        self._check(fn(
            self._ctx, in_tensor.data_ptr(), stride, msg_len, n,
            out_tensor.data_ptr()))
        return out_tensor

    def stats(self) -> dict:
        s = SreStats()
        self._check(self._lib.sre_get_stats(self._ctx, ctypes.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in SreStats._fields_}

    def path_counters(self) -> dict:
        """Which branch-pipeline paths the last root-type call took
        (include/sre.h sre_get_path_counters)."""
        out = (ctypes.c_uint64 * 4)()
        self._check(self._lib.sre_get_path_counters(self._ctx, out))
        return {"class_levels": out[0], "fused_groups": out[1],
                "chunks": out[2], "pipe2_levels": out[3]}

    def incremental_counters(self) -> dict:
        """What the last incremental_root / incremental_root_with_updates
        call reused and recomputed (include/sre.h
        sre_get_incremental_counters)."""
        out = (ctypes.c_uint64 * 6)()
        self._check(self._lib.sre_get_incremental_counters(self._ctx, out))
        return {"examined": out[0], "seeded": out[1], "rehashed": out[2],
                "small_acct_merge": out[3], "small_st_merge": out[4],
                "captured": out[5]}

    # ---- revert capture and unwind ----
    def capture_reverts(self, on: bool):
        """Turn revert capture on or off (off by default). While on, every
        successful apply_delta / incremental_root /
        incremental_root_with_updates / root_from_nodes also stores the
        delta that undoes it (include/sre.h sre_set_revert_capture); only
        the last one is kept. Turning it off drops the stored revert."""
        self._check(self._lib.sre_set_revert_capture(
            self._ctx, 1 if on else 0))

    def revert_counts(self):
        """(account rows, storage rows) of the stored revert; (0, 0) when
        none is stored."""
        return self._counts(self._lib.sre_revert_counts)

    def revert(self):
        """The stored revert as (DELTA_DTYPE array, STORAGE_DTYPE array): a
        valid delta over the current state that restores, row for row, the
        state before the last captured delta. Keep it to unwind more than
        one block: apply the fetched reverts newest first through
        incremental_root."""
        na, ns = self.revert_counts()
        acct = np.zeros(na, dtype=DELTA_DTYPE)
        st = np.zeros(ns, dtype=STORAGE_DTYPE)
        self._check(self._lib.sre_revert_get(
            self._ctx, _np_ptr(acct), na, _np_ptr(st), ns))
        return acct, st

    def unwind(self) -> bytes:
        """incremental_root over the stored revert: the resident state and
        the root go back to before the last captured delta (the unwind of
        MerkleStage). With capture on, the stored revert becomes the redo.
        Raises with `no-revert-captured` when nothing is stored."""
        return self._root(self._lib.sre_unwind)

    def unwind_with_updates(self):
        """incremental_root_with_updates over the stored revert: (root, net
        row diff against the trie before the unwind)."""
        root = self._root(self._lib.sre_unwind_with_updates)
        return root, self._fetch_updates()

    def revert_counters(self) -> dict:
        """What the last revert capture did (include/sre.h
        sre_get_revert_counters)."""
        out = (ctypes.c_uint64 * 4)()
        self._check(self._lib.sre_get_revert_counters(self._ctx, out))
        return {"acct_rows": out[0], "st_rows": out[1], "wiped_rows": out[2],
                "no_row": out[3]}
