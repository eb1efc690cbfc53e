"""The "Failed calls" contract of include/sre.h as a key-only model, and
builders for every kind of delta it rejects (CPU-only; no engine import).

States are `{key: [nonce, balance, code_hash, {slot: int}]}` dicts (the
shape tests.test_gpu_incremental._arrays_of takes). A delta is a pair
`(rows, strows)` in the `_mk_delta` form, but its order is part of the
input here: rows and strows are lists in exactly the order the engine is
to see them, so an unsorted delta can be written down.

`verdict()` restates which deltas the header rejects and with which token.
It knows keys and values only, nothing of merge paths or kernels.

Every builder returns a `Case`: the bad delta, the token the header
promises for it, and a good twin with the same `(n_acct, n_st, destroyed)`
shape. The merge path the engine picks depends on exactly these counts (and
on the resident state), so the twin takes the path the bad delta would have
taken; the GPU tests read the path off the twin's counters.
"""
import collections

from oracle import bind, pyref

KE = pyref.KECCAK_EMPTY

# tokens of include/sre.h "Failed calls"
T_ACCT = "accounts-not-sorted"
T_ST = "storage-not-sorted-or-duplicate"
T_ORPHAN = "storage-for-unknown-account"

Case = collections.namedtuple("Case", "kind token bad twin")


def verdict(accounts, rows, strows):
    """None if (rows, strows) is a valid delta over `accounts`, else the
    token its rejection message must contain. sre.h "Failed calls":
      - unsorted/duplicate account rows           -> accounts-not-sorted
      - unsorted/duplicate (acct, slot) rows      -> storage-not-sorted-or-duplicate
      - any storage row for an account the delta destroys,
        or a NONZERO row for an account that is neither resident nor
        upserted by the delta                     -> storage-for-unknown-account
    A zero-valued row for an unknown account is a no-op deletion."""
    for a, b in zip(rows, rows[1:]):
        if a[0] >= b[0]:
            return T_ACCT
    for a, b in zip(strows, strows[1:]):
        if (a[0], a[1]) >= (b[0], b[1]):
            return T_ST
    destroyed = {r[0] for r in rows if r[4]}
    upserted = {r[0] for r in rows if not r[4]}
    for ak, _, v in strows:
        if ak in destroyed:
            return T_ORPHAN
        if v != 0 and ak not in upserted and ak not in accounts:
            return T_ORPHAN
    return None


def shape(delta):
    rows, strows = delta
    return len(rows), len(strows), sum(1 for r in rows if r[4])


def apply(accounts, delta):
    """Overlay semantics of sre_apply_delta on the dict, for VALID deltas:
    post-state wins, an upsert keeps the account's storage, a deleted
    account disappears with its storage, a zero value deletes the slot."""
    rows, strows = delta
    assert verdict(accounts, rows, strows) is None
    for k, n, b, ch, dead in rows:
        if dead:
            accounts.pop(k, None)
        else:
            slots = accounts[k][3] if k in accounts else {}
            accounts[k] = [n, b, ch, slots]
    for ak, sk, v in strows:
        if v:
            accounts[ak][3][sk] = v
        elif ak in accounts:
            accounts[ak][3].pop(sk, None)


def n_slots(accounts):
    return sum(len(v[3]) for v in accounts.values())


# ---- pieces ---------------------------------------------------------------

def _bump(accounts, k, by):
    n, b, ch, _ = accounts[k]
    return (k, n, b + by, ch, 0)


def _pick(accounts, rng, n, want_slots=False, avoid=()):
    """n distinct resident keys, ascending"""
    pool = [k for k in sorted(accounts)
            if k not in avoid and (accounts[k][3] or not want_slots)]
    idx = rng.choice(len(pool), n, replace=False)
    return sorted(pool[int(i)] for i in idx)


def _fresh_slot(tag, *parts):
    return bind.keccak256(b"dc-slot" + tag + b"".join(parts))


def _fresh_account(accounts, tag):
    """A non-resident key in the lower half of the key order, so inserting
    it shifts the array position of at least half the resident accounts."""
    keys = sorted(accounts)
    for i in range(64):
        k = bind.keccak256(b"dc-acct" + tag + bytes([i]))
        if k not in accounts and k < keys[len(keys) // 2]:
            return k
    raise AssertionError("no fresh key in the lower half")


def _rider(accounts, rng, tag, avoid):
    """One valid slot upsert on a storage-bearing account, for deltas whose
    defect is on the account side: over a state with storage the delta then
    reaches a storage merge (and not the keep-storage shortcut)."""
    if not n_slots(accounts):
        return []
    (c,) = _pick(accounts, rng, 1, want_slots=True, avoid=avoid)
    return [(c, _fresh_slot(tag, c[:4]), 7)]


def unknown_key(accounts, where):
    """A key of no resident account: before every account key, between two
    adjacent ones, or after the last."""
    keys = sorted(accounts)
    if where == "before":
        u = bytes(31) + b"\x01"
        assert u < keys[0]
    elif where == "after":
        u = b"\xff" * 32
        assert u > keys[-1]
    else:
        lo = keys[len(keys) // 3]
        u = (int.from_bytes(lo, "big") + 1).to_bytes(32, "big")
        assert lo < u < keys[len(keys) // 3 + 1]
    assert u not in accounts
    return u


# ---- the rejected kinds ---------------------------------------------------

def k1_accounts_swapped(accounts, rng):
    a, b = _pick(accounts, rng, 2)
    st = _rider(accounts, rng, b"k1", (a, b))
    good = [_bump(accounts, a, 3), _bump(accounts, b, 5)]
    return Case("K1", T_ACCT, (good[::-1], st), (good, st))


def k2_account_duplicate(accounts, rng):
    a, b = _pick(accounts, rng, 2)
    st = _rider(accounts, rng, b"k2", (a, b))
    bad = [_bump(accounts, a, 3), _bump(accounts, a, 4)]
    good = [_bump(accounts, a, 3), _bump(accounts, b, 4)]
    return Case("K2", T_ACCT, (bad, st), (good, st))


def k3_slots_swapped_within(accounts, rng):
    (c,) = _pick(accounts, rng, 1)
    s1, s2 = sorted([_fresh_slot(b"k3a", c[:4]), _fresh_slot(b"k3b", c[:4])])
    good = [(c, s1, 11), (c, s2, 12)]
    return Case("K3-within", T_ST, ([], good[::-1]), ([], good))


def k3_slots_swapped_across(accounts, rng):
    c, d = _pick(accounts, rng, 2)
    # the slot keys alone are ascending: only the account keys are out of order
    s1, s2 = sorted([_fresh_slot(b"k3c", c[:4]), _fresh_slot(b"k3d", d[:4])])
    bad = [(d, s1, 11), (c, s2, 12)]
    return Case("K3-across", T_ST, ([], bad), ([], sorted(bad)))


def k4_slot_duplicate(accounts, rng):
    (c,) = _pick(accounts, rng, 1)
    s1, s2 = sorted([_fresh_slot(b"k4a", c[:4]), _fresh_slot(b"k4b", c[:4])])
    return Case("K4", T_ST, ([], [(c, s1, 5), (c, s1, 6)]),
                ([], [(c, s1, 5), (c, s2, 6)]))


def k5_row_for_destroyed(accounts, rng):
    c, d = _pick(accounts, rng, 2)
    rows = [(c, 0, 0, KE, 1)]
    return Case("K5", T_ORPHAN, (rows, [(c, _fresh_slot(b"k5", c[:4]), 9)]),
                (rows, [(d, _fresh_slot(b"k5", d[:4]), 9)]))


def k6_row_for_unknown(accounts, rng, where):
    """Nonzero row for an account that is neither resident nor upserted.
    The delta also inserts one fresh account (positions shift) and never
    deletes: on an engine that adopted this delta before rejecting it, the
    retained positions would be stale but still in range."""
    u = unknown_key(accounts, where)
    f = _fresh_account(accounts, b"k6" + where.encode())
    assert f != u
    (c,) = _pick(accounts, rng, 1)
    rows = [(f, 1, 7, KE, 0)]
    return Case("K6-" + where, T_ORPHAN,
                (rows, [(u, _fresh_slot(b"k6", u[:4]), 9)]),
                (rows, [(c, _fresh_slot(b"k6", c[:4]), 9)]))


KINDS = collections.OrderedDict([
    ("K1", k1_accounts_swapped),
    ("K2", k2_account_duplicate),
    ("K3-within", k3_slots_swapped_within),
    ("K3-across", k3_slots_swapped_across),
    ("K4", k4_slot_duplicate),
    ("K5", k5_row_for_destroyed),
    ("K6-before", lambda a, r: k6_row_for_unknown(a, r, "before")),
    ("K6-between", lambda a, r: k6_row_for_unknown(a, r, "between")),
    ("K6-after", lambda a, r: k6_row_for_unknown(a, r, "after")),
])
ACCOUNT_KINDS = ("K1", "K2")  # the only ones an accounts-only delta can show


# ---- accepted controls ----------------------------------------------------

def c1_zero_row_for_unknown(accounts, rng):
    """no-op deletion: accepted, and the state does not change"""
    u = unknown_key(accounts, "between")
    return [], [(u, _fresh_slot(b"c1", u[:4]), 0)]


def c2_row_for_inserted(accounts, rng):
    f = _fresh_account(accounts, b"c2")
    return [(f, 1, 7, KE, 0)], [(f, _fresh_slot(b"c2", f[:4]), 9)]


CONTROLS = collections.OrderedDict([
    ("C1", c1_zero_row_for_unknown),
    ("C2", c2_row_for_inserted),
])


# ---- good deltas for chains -----------------------------------------------

def good_delta(accounts, rng, step, max_st=3):
    """One valid delta of a rotating flavour — slot upsert + slot delete;
    a destroyed storage-bearing account + a slot upsert elsewhere; an
    inserted account with storage + a balance change — with at most
    `max_st` storage rows. Does not touch `accounts`."""
    assert max_st >= 1
    tag = b"gd" + bytes([step])
    rows, strows = [], []
    flavour = step % 3
    if flavour == 0:
        c, d = _pick(accounts, rng, 2, want_slots=True)
        strows = [(c, _fresh_slot(tag, c[:4]), 100 + step),
                  (d, sorted(accounts[d][3])[0], 0),
                  (d, _fresh_slot(tag, d[:4]), 200 + step)]
    elif flavour == 1:
        victim, c = _pick(accounts, rng, 2, want_slots=True)
        rows = [(victim, 0, 0, KE, 1)]
        strows = [(c, _fresh_slot(tag, c[:4]), 300 + step),
                  (c, sorted(accounts[c][3])[-1], 0)]
    else:
        f = _fresh_account(accounts, tag)
        (c,) = _pick(accounts, rng, 1)
        rows = sorted([(f, 1, 40 + step, KE, 0), _bump(accounts, c, 17)])
        strows = [(f, _fresh_slot(tag, b"a"), 400 + step),
                  (f, _fresh_slot(tag, b"b"), 500 + step)]
    return rows, sorted(strows[:max_st])
