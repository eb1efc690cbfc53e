"""Deliberately built small states that sit on RLP / keccak-block length
boundaries (CPU-only builders; no engine import).

Every builder returns (accounts, labels): `accounts` is a list of
(hashed_key, (nonce, balance, code_hash, {hashed_slot: int})) like the
adversarial-shape builders, `labels` maps each account key to a short
string naming the case, so a parity failure can say which case broke.

Sizes quoted in comments are checked, not assumed: the non-vacuity tests
in test_rlp_corpus_cpu.py recompute every node length with oracle.pyref.
"""
import collections
import random

from oracle import bind, pyref

KE = pyref.KECCAK_EMPTY


def _nib_key(nibs):
    assert len(nibs) == 64
    return bytes((nibs[2 * i] << 4) | nibs[2 * i + 1] for i in range(32))


def value_of(rng, length, hi):
    """A U256 whose minimal big-endian form is `length` bytes with the top
    byte >= 0x80 (hi) or in 1..0x7F."""
    top = rng.randrange(0x80, 0x100) if hi else rng.randrange(1, 0x80)
    return int.from_bytes(bytes([top]) + rng.randbytes(length - 1), "big")


# --------------------------------------------------------------------------
# storage-leaf grid
# --------------------------------------------------------------------------

GRID_DS = list(range(-1, 64))


def grid_cases():
    """(L, cls, value-or-None) per shared depth: lengths 2..32 in both
    top-byte classes, length 1 as exactly 0x01, 0x7F, 0x80, 0xFF."""
    cases = [(1, "lo", 0x01), (1, "lo", 0x7F), (1, "hi", 0x80),
             (1, "hi", 0xFF)]
    for L in range(2, 33):
        cases += [(L, "lo", None), (L, "hi", None)]
    return cases


def storage_leaf_grid(seed=20240613):
    """One account per (D, L, class): a storage trie of two slots sharing
    exactly D nibbles (D = -1: one slot). One slot holds a value of
    minimal length L in the named class, the other length 33-L in the
    other class. Both leaves therefore have max-neighbour-lcp D, which is
    what selects the leaf kernel's register path (D <= 13) or its LDS path.
    labels[key] = (D, L, cls, value)."""
    rng = random.Random(seed)
    accounts, labels = [], {}
    for D in GRID_DS:
        for L, cls, fixed in grid_cases():
            v = fixed if fixed is not None else value_of(rng, L, cls == "hi")
            a = [rng.randrange(16) for _ in range(64)]
            slots = {_nib_key(a): v}
            if D >= 0:
                b = a[:D] + [(a[D] + rng.randrange(1, 16)) % 16] + \
                    [rng.randrange(16) for _ in range(63 - D)]
                slots[_nib_key(b)] = value_of(rng, 33 - L, cls != "hi")
            key = bind.keccak256(b"leafgrid" + bytes([D + 1, L]) +
                                 cls.encode() + v.to_bytes(32, "big"))
            accounts.append((key, (1, 1, KE, slots)))
            labels[key] = (D, L, cls, v)
    return accounts, labels


def storage_leaf_len(slot_key, value, D):
    """RLP length of the leaf for slot_key below a branch at depth D."""
    item = (pyref.nibbles_of(slot_key), pyref.rlp_int(value))
    return len(pyref._build([item], D + 1))


# --------------------------------------------------------------------------
# account-leaf grid
# --------------------------------------------------------------------------

NONCES = {0: [0], 1: [1, 0x7F, 0x80, 0xFF], 8: [1 << 56, (1 << 64) - 1]}


def nonces_of_len(n):
    if n in NONCES:
        return NONCES[n]
    return [1 << (8 * (n - 1)), (1 << (8 * n)) - 1]


def account_leaf_grid(nonce_len, seed=77):
    """One state per nonce byte length: every balance byte length 0..32 in
    both top-byte classes, for each nonce of that length. No storage
    (storage root = EMPTY_ROOT_HASH); code hash alternates between
    KECCAK_EMPTY and a real hash. labels[key] = (nonce, balance)."""
    rng = random.Random((seed << 8) | nonce_len)
    accounts, labels = [], {}
    i = 0
    for nonce in nonces_of_len(nonce_len):
        for bl in range(33):
            for hi in ([False] if bl == 0 else [False, True]):
                bal = 0 if bl == 0 else value_of(rng, bl, hi)
                if nonce == 0 and bal == 0:
                    # reth never stores an empty account; give it code
                    ch = bind.keccak256(b"code0")
                else:
                    ch = KE if i % 2 else bind.keccak256(b"code" + bytes([i % 256]))
                key = bind.keccak256(b"acctgrid" + bytes([nonce_len]) +
                                     i.to_bytes(4, "big"))
                accounts.append((key, (nonce, bal, ch, {})))
                labels[key] = (nonce, bal)
                i += 1
    return accounts, labels


def account_leaf_lens(accounts):
    """Counter of account-leaf RLP lengths in the account trie of exactly
    these accounts (pyref)."""
    items = sorted((pyref.nibbles_of(k),
                    pyref.account_value(n, b, pyref.storage_root(s) if s
                                        else pyref.EMPTY_ROOT_HASH, ch))
                   for k, (n, b, ch, s) in accounts)
    return collections.Counter(
        len(rlp) for _, kind, _, rlp in pyref.iter_nodes(items, 0)
        if kind == "leaf")


def single_account_states():
    """Single-account states (D = -1). Root-form leaf (64-nibble key) RLP of
    exactly 135, 136, 137 and 138 bytes; the subtree child-ref form drops
    the top nibble's byte from the HP key, so the same four states give
    134..137 there — both emit forms cross the 136-byte block boundary.
    Leaf = 2 + 34 (HP item) + 2 + 2 + nonce_rlp + balance_rlp + 66."""
    out = []
    for total in (135, 136, 137, 138):
        bal_len = total - 106 - 1 - 1  # nonce 1 -> 1 B; balance 0x80+len
        bal = int.from_bytes(bytes([0x80 + total - 135]) +
                             bytes(range(1, bal_len)), "big")
        key = bind.keccak256(b"single" + bytes([total]))
        out.append((total, [(key, (1, bal, KE, {}))]))
    return out


# --------------------------------------------------------------------------
# branch-length states
# --------------------------------------------------------------------------

def _leaf_ref_table(rem):
    """{ref size: (L, hi)} for a storage leaf with `rem` remaining key
    nibbles: the sizes a child of a deep branch can take."""
    nib = tuple([0] * (64 - rem) + [1] * rem)
    table = {}
    for L in range(1, 33):
        for hi in (False, True):
            top = 0x80 if hi else 0x01
            v = int.from_bytes(bytes([top]) + b"\x11" * (L - 1), "big")
            rlp = pyref._build([(nib, pyref.rlp_int(v))], 64 - rem)
            size = len(rlp) if len(rlp) < 32 else 33
            table.setdefault(size, (L, hi))
    return table


def _solve(k, total, sizes):
    """k ref sizes from `sizes` (descending preference) summing to total."""
    lo, hi = min(sizes), max(sizes)
    memo = {}

    def go(k, total):
        if k == 0:
            return [] if total == 0 else None
        if total < k * lo or total > k * hi:
            return None
        if (k, total) in memo:
            return memo[(k, total)]
        res = None
        for s in sizes:
            rest = go(k - 1, total - s)
            if rest is not None:
                res = [s] + rest
                break
        memo[(k, total)] = res
        return res

    return go(k, total)


# (name, shared nibbles, children, branch-RLP length, inline children only)
# payload = (17 - k) + sum(refs); header 1 B below 56, 2 B to 255, then 3 B.
BRANCH_TARGETS = [
    # total 31/32/33: inline ref vs hashed. 31 needs one 6-byte child,
    # which a 7-nibble leaf cannot be (7 + 8 is not a reachable pair at
    # depth 56), so that one shares 58 nibbles (5-nibble leaves).
    ("t31", 58, 2, 31, True),
    ("t32", 56, 2, 32, True),
    ("t33", 56, 2, 33, True),
    # payload 55/56: the list header grows from 1 to 2 bytes
    ("p55", 56, 3, 56, False),
    ("p56", 56, 3, 58, False),
    # one/two keccak blocks, few members (class 1) ...
    ("t135_k4", 56, 4, 135, False),
    ("t136_k5", 56, 5, 136, False),
    ("t137_k7", 56, 7, 137, False),
    # ... and many mostly-inline members (class 3, but two blocks at most)
    ("t135_k12", 56, 12, 135, True),
    ("t136_k13", 56, 13, 136, True),
    ("t137_k16", 56, 16, 137, True),
    # payload 255/256: header 2 -> 3 bytes
    ("p255", 56, 8, 257, False),
    ("p256", 56, 8, 259, False),
    # two/three blocks
    ("t271", 56, 8, 271, False),
    ("t272", 56, 9, 272, False),
    ("t273", 56, 11, 273, False),
    # three/four blocks
    ("t407", 56, 13, 407, False),
    ("t408", 56, 14, 408, False),
    ("t409", 56, 16, 409, False),
    # 16 hashed children: the largest branch there is (532 B)
    ("max", 56, 16, 532, False),
    # all-inline fans: class 3 / class 2 by member count, one block by size;
    # and a 2-child all-inline branch that is itself inline in its parent
    ("inl16", 56, 16, 2 + 1 + 16 * 7, True),
    ("inl12", 56, 12, 2 + 5 + 12 * 7, True),
    ("inl2", 56, 2, 1 + 15 + 2 * 7, True),
]
BRANCH_LENGTHS = sorted({t[3] for t in BRANCH_TARGETS})


def _branch_trie(rng, share, k, total, inline_only):
    """Storage slots sharing `share` nibbles, then a k-child branch whose
    RLP is `total` bytes. The shared prefix puts an extension node above
    the branch."""
    table = _leaf_ref_table(63 - share)
    hdr = 1 if total - 1 < 56 else 2 if total - 2 <= 255 else 3
    payload = total - hdr
    assert (hdr, payload < 56, payload <= 255) in \
        [(1, True, True), (2, False, True), (3, False, False)], total
    sizes = sorted((s for s in table if not (inline_only and s == 33)),
                   reverse=True)
    refs = _solve(k, payload - (17 - k), sizes)
    assert refs is not None, (share, k, total)
    rng.shuffle(refs)
    prefix = [rng.randrange(16) for _ in range(share)]
    slots = {}
    for nib, size in zip(sorted(rng.sample(range(16), k)), refs):
        L, hi = table[size]
        if size == 33:
            L = rng.randrange(L, 33)  # any longer value is hashed too
        tail = [rng.randrange(16) for _ in range(63 - share)]
        slots[_nib_key(prefix + [nib] + tail)] = value_of(rng, L, hi)
    return slots


def branch_length_tries(seed=5150):
    """{name: slots}: one storage trie per BRANCH_TARGETS row."""
    rng = random.Random(seed)
    return {name: _branch_trie(rng, share, k, total, inl)
            for name, share, k, total, inl in BRANCH_TARGETS}


def branch_length_state(copies=28, seed=5150):
    """Every branch-length trie replicated under `copies` distinct account
    keys (same slot layout): 23 x 28 = 644 accounts, so the deep levels
    hold several hundred groups of mixed size class. labels[key] = name."""
    tries = branch_length_tries(seed)
    accounts, labels = [], {}
    for name, slots in tries.items():
        for c in range(copies):
            key = bind.keccak256(b"brlen" + name.encode() + bytes([c]))
            accounts.append((key, (c, 10 ** 18 + c, KE, dict(slots))))
            labels[key] = name
    return accounts, labels
