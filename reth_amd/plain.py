"""Deterministic PLAIN-state generator: unhashed rows for upload_plain /
set_plain_device_tensors (include/sre.h sre_plain_account /
sre_plain_storage). numpy and torch forms produce the same rows
(tests/test_plain_model_cpu.py).

Spec, on the splitmix of reth_amd.gen (same SEED and constants):

  account counter c in [first, first + n_accounts):
    address    = LE64(splitmix(c ^ S_ADDR[0])) || LE64(splitmix(c ^ S_ADDR[1]))
                 || the low 4 bytes of LE64(splitmix(c ^ S_ADDR[2]))
    nonce, balance, code_hash: as reth_amd.gen gives counter c
  slot j in [0, slots(c)) of account c, x = c << 32 | j:
    slot       = LE64(splitmix(x ^ S_SLOT[k])), k = 0..3
    value      = as reth_amd.gen gives (c, j)

Rows come out in counter order, storage grouped by account with j
ascending: the order of reth's PlainAccountState / PlainStorageState is by
address, which for hashing purposes is just "some order". `slots` is one
count for every account or one count per account.
"""
import numpy as np

from reth_amd import gen
from reth_amd.engine import PLAIN_ACCOUNT_DTYPE, PLAIN_STORAGE_DTYPE

S_ADDR = [0xB1AC5EED0000A000 + k for k in range(3)]
S_SLOT = [0xB1AC5EED0000B000 + k for k in range(4)]


# ---------------------------------------------------------------------------
# numpy
# ---------------------------------------------------------------------------

def _counts_np(n_accounts, slots):
    if np.ndim(slots) == 0:
        return np.full(n_accounts, int(slots), dtype=np.int64)
    counts = np.asarray(slots, dtype=np.int64)
    assert counts.shape == (n_accounts,)
    return counts


def gen_plain_numpy(n_accounts, slots, first=0):
    """-> (PLAIN_ACCOUNT_DTYPE array, PLAIN_STORAGE_DTYPE array)."""
    old = np.seterr(over="ignore")
    try:
        sm, le, be = gen._sm64_np, gen._np_le64, gen._np_be64
        c = np.arange(first, first + n_accounts, dtype=np.uint64)
        acct = np.zeros(n_accounts, dtype=PLAIN_ACCOUNT_DTYPE)
        addr = np.zeros((n_accounts, 24), dtype=np.uint8)
        for k in range(3):
            addr[:, 8 * k:8 * (k + 1)] = le(sm(c ^ np.uint64(S_ADDR[k])))
        acct["address"] = addr[:, :20]
        acct["nonce"] = c & np.uint64(0xFFFF)
        bal = np.zeros((n_accounts, 32), dtype=np.uint8)
        bal[:, 16:24] = be(sm(c ^ np.uint64(gen.S_BAL_HI)) | np.uint64(1))
        bal[:, 24:32] = be(sm(c ^ np.uint64(gen.S_BAL_LO)))
        acct["balance"] = bal
        ch = np.tile(np.frombuffer(gen.KECCAK_EMPTY, np.uint8),
                     (n_accounts, 1)).copy()
        rare = (sm(c ^ np.uint64(gen.S_CODE)) % np.uint64(10)) >= np.uint64(9)
        for k in range(4):
            v = le(sm(c ^ np.uint64(gen.S_CH[k])))
            ch[rare, 8 * k:8 * (k + 1)] = v[rare]
        acct["code_hash"] = ch

        counts = _counts_np(n_accounts, slots)
        ns = int(counts.sum())
        st = np.zeros(ns, dtype=PLAIN_STORAGE_DTYPE)
        if ns:
            cc = np.repeat(c, counts)
            starts = np.cumsum(counts) - counts
            jj = (np.arange(ns, dtype=np.int64)
                  - np.repeat(starts, counts)).astype(np.uint64)
            st["address"] = np.repeat(addr[:, :20], counts, axis=0)
            x = (cc << np.uint64(32)) | jj
            slot = np.zeros((ns, 32), dtype=np.uint8)
            for k in range(4):
                slot[:, 8 * k:8 * (k + 1)] = le(sm(x ^ np.uint64(S_SLOT[k])))
            st["slot"] = slot
            xv = x ^ np.uint64(gen.S_VAL)
            L = (np.uint64(1) + (sm(xv) & np.uint64(31))).astype(np.int64)
            top = (np.uint64(1) + sm(xv ^ np.uint64(gen.S_VB)) % np.uint64(255)
                   ).astype(np.uint8)
            body = np.zeros((ns, 32), dtype=np.uint8)
            for k in range(4):
                body[:, 8 * k:8 * (k + 1)] = le(sm(xv ^ np.uint64(gen.S_VK[k])))
            colim = np.arange(32)[None, :]
            vals = np.where(colim >= (32 - L)[:, None], body, 0).astype(np.uint8)
            vals[np.arange(ns), 32 - L] = top
            st["value"] = vals
        return acct, st
    finally:
        np.seterr(**old)


# ---------------------------------------------------------------------------
# torch (bench-scale generation on the device; also runs on CPU)
# ---------------------------------------------------------------------------

def gen_plain_torch(n_accounts, slots, device="cuda", first=0):
    """-> (acct (na,96) u8, st (ns,84) u8) tensors laid out as
    sre_plain_account / sre_plain_storage. slots: int or (na,) int64
    tensor."""
    import torch
    sm, le, be, i64 = gen._sm64_t, gen._bytes_le, gen._bytes_be, gen._i64
    c = torch.arange(first, first + n_accounts, dtype=torch.int64, device=device)
    acct = torch.zeros((n_accounts, 96), dtype=torch.uint8, device=device)
    addr = torch.cat([le(sm(c ^ i64(S_ADDR[k]))) for k in range(3)],
                     dim=1)[:, :20].contiguous()
    acct[:, 0:20] = addr
    acct[:, 24:32] = le(c & 0xFFFF)
    acct[:, 48:56] = be(sm(c ^ i64(gen.S_BAL_HI)) | 1)
    acct[:, 56:64] = be(sm(c ^ i64(gen.S_BAL_LO)))
    ke = torch.tensor(list(gen.KECCAK_EMPTY), dtype=torch.uint8, device=device)
    ch = ke.repeat(n_accounts, 1)
    rare = gen._umod(sm(c ^ i64(gen.S_CODE)), 10) >= 9
    for k in range(4):
        v = le(sm(c ^ i64(gen.S_CH[k])))
        ch[:, 8 * k:8 * (k + 1)] = torch.where(rare[:, None], v,
                                               ch[:, 8 * k:8 * (k + 1)])
    acct[:, 64:96] = ch

    if isinstance(slots, int):
        counts = torch.full((n_accounts,), slots, dtype=torch.int64,
                            device=device)
    else:
        counts = slots.to(device=device, dtype=torch.int64)
    ns = int(counts.sum().item()) if n_accounts else 0
    st = torch.zeros((ns, 84), dtype=torch.uint8, device=device)
    if ns:
        cc = c.repeat_interleave(counts)
        starts = torch.cumsum(counts, 0) - counts
        jj = torch.arange(ns, dtype=torch.int64, device=device) \
            - starts.repeat_interleave(counts)
        st[:, 0:20] = addr.repeat_interleave(counts, dim=0)
        x = (cc << 32) | jj
        del cc, jj, starts
        for k in range(4):
            st[:, 20 + 8 * k:28 + 8 * k] = le(sm(x ^ i64(S_SLOT[k])))
        xv = x ^ i64(gen.S_VAL)
        del x
        L = (1 + (sm(xv) & 31)).to(torch.int64)
        top = (1 + gen._umod(sm(xv ^ i64(gen.S_VB)), 255)).to(torch.uint8)
        body = torch.cat([le(sm(xv ^ i64(gen.S_VK[k]))) for k in range(4)], dim=1)
        del xv
        colim = torch.arange(32, device=device)[None, :]
        vals = torch.where(colim >= (32 - L)[:, None], body,
                           torch.zeros_like(body))
        del body
        vals[torch.arange(ns, device=device), 32 - L] = top
        st[:, 52:84] = vals
    return acct, st


def np_plain_to_tensors(acct, st, device="cpu"):
    """numpy structured arrays -> raw (na,96)/(ns,84) uint8 tensors."""
    import torch
    a = torch.from_numpy(acct.view(np.uint8).reshape(len(acct), 96).copy())
    s = torch.from_numpy(st.view(np.uint8).reshape(len(st), 84).copy())
    return a.to(device), s.to(device)


def tensors_to_np_plain(acct_u8, st_u8):
    """raw uint8 tensors (any device) -> numpy structured arrays."""
    a = acct_u8.cpu().numpy().reshape(-1).view(PLAIN_ACCOUNT_DTYPE)
    s = st_u8.cpu().numpy().reshape(-1).view(PLAIN_STORAGE_DTYPE)
    return a, s
