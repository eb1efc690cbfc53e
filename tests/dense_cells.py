"""Dense-cell states for the dirty-path incremental root (CPU-only builder;
no engine import).

The incremental root retains one record per populated 5-nibble cell that
has a sibling cell under the same 4-nibble prefix. Random
keccak keys at test sizes almost never put two accounts into one cell, so
this module builds keys as a chosen 5-nibble cell prefix followed by
keccak-derived nibbles: every retained record is then a real multi-account
subtree, and the account TrieUpdates rows below depth 4 live inside them.

States are `{key: [nonce, balance, code_hash, {slot: int}]}` dicts (the
shape tests.test_gpu_incremental._arrays_of takes). Scenarios are
generators that yield one delta at a time as `(rows, strows)` in the
`_mk_delta` form and expect the caller to apply it to the same dict before
resuming them.

`model()` is the reuse model, from keys only: which retained records a
delta must leave reusable, and therefore what the engine's incremental
counters must read. It restates the cell rules of DESIGN.md §9 and knows
nothing of the engine.
"""
import collections

from oracle import bind, pyref

KE = pyref.KECCAK_EMPTY

# ---- layout (cells are 20-bit ints, groups 16-bit) ------------------------
FULL = 0x3A7C                 # all 16 cells populated
FULL_BIG = FULL << 4 | 0x0    # 60 accounts: top branch stored
FULL_LEAF = FULL << 4 | 0x1   # 1 account: its retained record is a leaf
FULL_SMALL = FULL << 4 | 0x2  # 3 accounts on 3 nibbles: top not stored
FULL_EXT = FULL << 4 | 0x3    # 12 accounts sharing 10 nibbles: ext + branch
FULL_MID = FULL << 4 | 0x4    # 10 accounts (shrink / grow)
NEIGH = 0x3A7D                # shares 3 nibbles with FULL
NEIGH_A, NEIGH_GAP, NEIGH_B = NEIGH << 4 | 0x2, NEIGH << 4 | 0x5, NEIGH << 4 | 0x9
PAIR = 0x81B4                 # 2-cell sibling group
PAIR_BIG, PAIR_SMALL = PAIR << 4 | 0x3, PAIR << 4 | 0xA
LONE, LONE_SIB = 0xC5E61, 0xC5E68  # no sibling: never captured
EDGES = (0x00000, 0x00001, 0xFFFFE, 0xFFFFF)


def cell(k):
    return int.from_bytes(k[:3], "big") >> 4


def group(k):
    return cell(k) >> 4


def nibbles(k):
    return [(b >> s) & 0xF for b in k for s in (4, 0)]


def _from_nibbles(n):
    return bytes((n[2 * i] << 4) | n[2 * i + 1] for i in range(32))


def key_in(c, tag, fixed=()):
    """A key in cell `c`: 5 prefix nibbles, then `fixed` nibbles, then
    nibbles of keccak(tag)."""
    n = nibbles(bind.keccak256(b"dense" + c.to_bytes(4, "big") + tag))
    pre = [(c >> s) & 0xF for s in (16, 12, 8, 4, 0)] + list(fixed)
    n[:len(pre)] = pre
    return _from_nibbles(n)


def edge_key(c, high):
    """The lowest / highest key of cell `c`."""
    return _from_nibbles([(c >> s) & 0xF for s in (16, 12, 8, 4, 0)]
                         + [0xF if high else 0] * 59)


def key_after(k):
    """The key right after `k` as a 256-bit integer: it shares about 63
    nibbles with `k`, so it sorts strictly between `k` and any other
    neighbour."""
    return (int.from_bytes(k, "big") + 1).to_bytes(32, "big")


def _cell_sizes(scale):
    big = int(60 * scale)
    sizes = {FULL_BIG: big, FULL_LEAF: 1, FULL_SMALL: 3, FULL_EXT: 12,
             NEIGH_A: big - 4, NEIGH_B: 25, PAIR_BIG: big - 2, PAIR_SMALL: 8,
             LONE: big - 6, 0x00000: 12, 0x00001: 10, 0xFFFFE: 10,
             0xFFFFF: 12}
    for c in range(4, 16):
        sizes[FULL << 4 | c] = 10 + (c % 3) * 2 if c < 10 \
            else int((80 + (c % 4) * 10) * scale)
    return sizes


def build_state(scale=1.0, slots=False):
    """The standard state (about 1000 accounts at scale 1). With `slots`,
    account i of a cell gets (i * 5 + cell) % 9 storage slots."""
    accounts = {}
    for c, n in sorted(_cell_sizes(scale).items()):
        for i in range(n):
            tag = i.to_bytes(4, "big")
            if c == FULL_SMALL:
                k = key_in(c, tag, fixed=[i])
            elif c == FULL_EXT:
                k = key_in(c, tag, fixed=[7, 0, 7, 0, 7])
            else:
                k = key_in(c, tag)
            sl = {}
            if slots:
                for j in range((i * 5 + c) % 9):
                    sl[bind.keccak256(b"dslot" + k[:8] + bytes([j]))] = \
                        1 + j + (i << 9)
            accounts[k] = [i % 7, 10 ** 6 + i * 1009 + c, KE, sl]
    return accounts


# ---- reuse model (keys only) ----------------------------------------------

def populated(keys):
    return collections.Counter(cell(k) for k in keys)


def captured(keys):
    """Cells that get a retained record: populated, with at least one
    populated sibling cell in the same group."""
    pop = populated(keys)
    per_group = collections.Counter(c >> 4 for c in pop)
    return {c for c in pop if per_group[c >> 4] >= 2}


def model(pre_keys, post_keys, rows, strows):
    """Expected incremental counters for one delta. `reused` is every cell
    captured before the delta that no delta key touches and that still
    has a sibling afterwards."""
    dirty = {cell(r[0]) for r in rows} | {cell(r[0]) for r in strows}
    cap_pre, cap_post = captured(pre_keys), captured(post_keys)
    reused = {c for c in cap_pre if c not in dirty and c in cap_post}
    return {"examined": len(cap_pre), "seeded": len(reused),
            "rehashed": sum(1 for k in post_keys if cell(k) not in reused),
            "captured": len(cap_post), "reused": reused, "dirty": dirty}


# ---- delta helpers --------------------------------------------------------

def keys_of(accounts, c):
    return sorted(k for k in accounts if cell(k) == c)


def mod(accounts, k, bump=1):
    v = accounts[k]
    return (k, v[0] + 1, v[1] + bump, v[2], 0)


def ins(k, seq=0):
    return (k, 1 + seq, 777000 + seq, KE, 0)


def dele(k):
    return (k, 0, 0, KE, 1)


def deep_key(accounts, c):
    """A key of cell `c` that shares at least 6 nibbles with a neighbour in
    the cell: it hangs below a branch under the cell top, so changing it
    changes a hash the cell-top row embeds."""
    ks = keys_of(accounts, c)
    for a, b in zip(ks, ks[1:]):
        if nibbles(a)[:6] == nibbles(b)[:6]:
            return a
    raise AssertionError(f"cell {c:05x} has no two keys sharing 6 nibbles")


def apply_rows(accounts, rows, strows=()):
    """The overlay semantics on the dict: post-state wins and keeps storage,
    a deleted account loses it, a zero slot value deletes the slot."""
    for (k, n, b, ch, dead) in rows:
        if dead:
            accounts.pop(k, None)
        else:
            old = accounts.get(k)
            accounts[k] = [n, b, ch, old[3] if old else {}]
    for (a, s, v) in strows:
        if v:
            accounts[a][3][s] = v
        else:
            accounts[a][3].pop(s, None)


def walk(accounts, scenario):
    """Run `scenario` over `accounts` (mutated in place). Per delta, after
    applying it to the dict, yields (rows, strows, expected) with
    `expected` from model() plus the pre-delta sizes (`na_pre`, `ns_pre`)
    and the deleted accounts that had storage (`destroyed`)."""
    for rows, strows in scenario(accounts):
        pre = list(accounts)
        ns_pre = sum(len(v[3]) for v in accounts.values())
        destroyed = {r[0] for r in rows
                     if r[4] and r[0] in accounts and accounts[r[0]][3]}
        apply_rows(accounts, rows, strows)
        exp = model(pre, list(accounts), rows, strows)
        exp.update(na_pre=len(pre), ns_pre=ns_pre, destroyed=destroyed)
        yield sorted(rows), sorted(strows), exp


def deep_account_rows(rowmap):
    """{row key: 5-nibble cell} of the account rows at path_len >= 5 among
    the keys of a tests.test_gpu_incremental_updates._rowmap."""
    return {k: int.from_bytes(k[3][:3], "big") >> 4
            for k in rowmap if k[0] == 0 and k[2] >= 5}


# ---- account scenarios: generators of (rows, strows), >= 4 deltas each ----

def sc_modify_in_full_group(acc):
    # 15 siblings reused; the depth-4 parent row embeds their retained hash
    yield [mod(acc, deep_key(acc, FULL_BIG))], []
    yield [mod(acc, keys_of(acc, FULL_LEAF)[0])], []
    yield [mod(acc, keys_of(acc, FULL_EXT)[3])], []
    yield [mod(acc, deep_key(acc, FULL << 4 | 0xF)),
           mod(acc, deep_key(acc, FULL_BIG))], []


def sc_insert_first_last_of_cell(acc):
    c = FULL << 4 | 0xB
    yield [ins(edge_key(c, False)), ins(edge_key(c, True), 1)], []
    yield [dele(edge_key(c, False)), dele(edge_key(c, True))], []
    ks = keys_of(acc, c)
    yield [ins(key_after(ks[0])), ins(key_after(ks[-1]), 1)], []
    yield [mod(acc, key_after(ks[0])), dele(ks[0])], []


def sc_new_cell_between_siblings(acc):
    # the neighbours stay clean while positions to their right shift
    yield [ins(key_in(NEIGH_GAP, b"n0"))], []
    yield [ins(key_in(NEIGH_GAP, b"n1"), 1), ins(key_in(NEIGH_GAP, b"n2"), 2)], []
    yield [dele(k) for k in keys_of(acc, NEIGH_GAP)], []
    yield [mod(acc, deep_key(acc, NEIGH_A))], []


def sc_delete_one_cell_of_pair(acc):
    # the survivor's junction moves: revalidation must miss
    yield [dele(k) for k in keys_of(acc, PAIR_SMALL)], []
    yield [mod(acc, deep_key(acc, PAIR_BIG))], []
    yield [ins(key_in(PAIR_SMALL, b"p0")), ins(key_in(PAIR_SMALL, b"p1"), 1)], []
    yield [mod(acc, deep_key(acc, PAIR_BIG))], []


def sc_lone_cell_gets_sibling(acc):
    yield [ins(key_in(LONE_SIB, b"s0"))], []
    yield [mod(acc, deep_key(acc, LONE))], []
    yield [dele(key_in(LONE_SIB, b"s0"))], []
    yield [mod(acc, deep_key(acc, LONE))], []


def sc_shrink_then_grow(acc):
    ks = keys_of(acc, FULL_MID)
    yield [dele(k) for k in ks[1:]], []
    yield [mod(acc, ks[0])], []
    yield [ins(k, i) for i, k in enumerate(ks[1:])], []
    yield [dele(ks[4]), mod(acc, ks[5])], []


def sc_small_cell_top_becomes_stored(acc):
    # a second key below nibble 0 of the 3-account cell turns that child
    # into a branch: the cell top becomes a stored row and the parent's
    # tree_mask bit flips; removing it flips it back
    twins = [key_in(FULL_SMALL, bytes([0x40 + i]), fixed=[0]) for i in range(3)]
    yield [ins(twins[0])], []
    yield [ins(twins[1], 1), ins(twins[2], 2)], []
    yield [dele(t) for t in twins], []
    yield [mod(acc, keys_of(acc, FULL_SMALL)[1])], []


def sc_first_and_last_cells(acc):
    lo, hi = keys_of(acc, 0x00000), keys_of(acc, 0xFFFFF)
    yield [mod(acc, lo[0]), mod(acc, hi[-1])], []
    yield [ins(edge_key(0x00000, False)), ins(edge_key(0xFFFFF, True), 1)], []
    yield [dele(edge_key(0x00000, False)), dele(edge_key(0xFFFFF, True))], []
    yield [dele(k) for k in keys_of(acc, 0x00001)], []
    yield [mod(acc, lo[1]), ins(key_after(hi[-1]))], []


def sc_full_group_down_to_two_cells(acc):
    keep = (FULL_BIG, FULL << 4 | 0x5)
    yield [dele(k) for k in sorted(acc)
           if group(k) == FULL and cell(k) not in keep], []
    yield [mod(acc, deep_key(acc, FULL_BIG))], []
    yield [dele(k) for k in keys_of(acc, keep[1])], []
    yield [ins(key_in(keep[1], b"back"))], []
    yield [mod(acc, deep_key(acc, FULL_BIG))], []


def sc_empty_and_idempotent(acc):
    yield [], []
    # identical values: the cells of the delta keys are still dirtied
    yield [(k, *acc[k][:3], 0) for c in (FULL_BIG, PAIR_BIG, LONE)
           for k in keys_of(acc, c)[:3]], []
    yield [], []
    yield [mod(acc, deep_key(acc, PAIR_BIG))], []


ACCOUNT_SCENARIOS = {f.__name__[3:]: f for f in (
    sc_modify_in_full_group, sc_insert_first_last_of_cell,
    sc_new_cell_between_siblings, sc_delete_one_cell_of_pair,
    sc_lone_cell_gets_sibling, sc_shrink_then_grow,
    sc_small_cell_top_becomes_stored, sc_first_and_last_cells,
    sc_full_group_down_to_two_cells, sc_empty_and_idempotent)}


# ---- storage scenarios (state built with slots=True) ----------------------

def _with_slots(acc, c, skip=()):
    return next(k for k in keys_of(acc, c) if acc[k][3] and k not in skip)


def sc_storage_only_then_destroy(acc):
    # every step carries at least one storage row, so the storage merge
    # runs on every step
    a = _with_slots(acc, FULL_BIG)
    yield [], [(a, bind.keccak256(b"st-new-0"), 41)]
    victim = _with_slots(acc, FULL_BIG, skip=(a,))
    b = _with_slots(acc, FULL << 4 | 0xE)
    yield [dele(victim)], [(b, sorted(acc[b][3])[0], 0),
                           (b, bind.keccak256(b"st-new-1"), 42)]
    yield [mod(acc, a)], [(a, bind.keccak256(b"st-new-0"), 43)]
    fresh = key_in(FULL_LEAF, b"st-acct")
    yield [ins(fresh), dele(_with_slots(acc, PAIR_BIG))], \
        [(fresh, bind.keccak256(b"st-new-2"), 44)]
    yield [], [(a, s, 0) for s in sorted(acc[a][3])[:2]]


STORAGE_SCENARIOS = {"storage_only_then_destroy": sc_storage_only_then_destroy}
