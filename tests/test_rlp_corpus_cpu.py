"""Non-vacuity of the RLP boundary corpora (tests/rlp_corpus.py): every
length the GPU boundary tests claim to exercise is recomputed here from
oracle.pyref alone, so a builder that silently misses its target fails on
the CPU before any kernel runs. The oracle and pyref must also agree on
the corpora, so the GPU tests compare against a reference that is itself
pinned."""
import numpy as np

from oracle import bind, pyref
from tests import rlp_corpus as rc
from tests.util import to_arrays


def _len_hi(v):
    """(minimal byte length, top byte >= 0x80) of a non-negative int."""
    L = (v.bit_length() + 7) // 8
    return L, L > 0 and (v >> (8 * (L - 1))) >= 0x80


def test_storage_leaf_grid_covers_both_leaf_paths():
    accounts, labels = rc.storage_leaf_grid()
    assert len(accounts) == 65 * 66
    seen = set()      # (D, value length, top-byte class)
    lens = {}         # D -> set of leaf RLP lengths
    for key, (_, _, _, slots) in accounts:
        D = labels[key][0]
        assert len(slots) == (1 if D < 0 else 2)
        ks = sorted(slots)
        if D >= 0:
            a, b = (pyref.nibbles_of(k) for k in ks)
            shared = next(i for i in range(64) if a[i] != b[i])
            assert shared == D, labels[key]
        for k in ks:
            v = slots[k]
            seen.add((D,) + _len_hi(v))
            lens.setdefault(D, set()).add(rc.storage_leaf_len(k, v, D))
    # the full cross product, on both sides of the D = 13/14 path switch
    for D in rc.GRID_DS:
        for L in range(1, 33):
            for hi in (False, True):
                assert (D, L, hi) in seen, (D, L, hi)
    vals = {labels[k][3] for k, _ in accounts if labels[k][1] == 1}
    assert vals == {0x01, 0x7F, 0x80, 0xFF}
    # one- and two-byte list headers on the register path, and inline
    # (< 32 B) leaves on it: D = 13 with a one-byte value
    assert min(lens[13]) < 32 <= max(lens[13])
    assert min(lens[0]) < 56 + 1 <= max(lens[0])
    assert max(lens[-1]) == 70  # the longest storage leaf there is
    # ... and long values right after the switch to the LDS path
    assert max(lens[14]) >= 32 and min(lens[14]) < 32


def test_storage_leaf_grid_oracle_matches_pyref_rows():
    accounts, labels = rc.storage_leaf_grid()
    acct, st = to_arrays(dict(accounts))
    got = bind.storage_roots(acct, st)
    rows = {-1, 0, 12, 13, 14, 62, 63}
    n = 0
    for i, a in enumerate(acct):
        key = bytes(a["key"])
        if labels[key][0] in rows:
            want = pyref.storage_root(dict(accounts)[key][3])
            assert bytes(got[i]) == want, labels[key]
            n += 1
    assert n == len(rows) * 66


def test_account_leaf_grid_reaches_the_block_boundary():
    all_lens = set()
    for nl in range(9):
        accounts, labels = rc.account_leaf_grid(nl)
        nonces = {n for n, _ in labels.values()}
        assert all((n.bit_length() + 7) // 8 == nl for n in nonces), nl
        bal_lens = {_len_hi(b) for _, b in labels.values()}
        for bl in range(1, 33):
            assert (bl, False) in bal_lens and (bl, True) in bal_lens, bl
        assert (0, False) in bal_lens
        lens = rc.account_leaf_lens(accounts)
        all_lens |= set(lens)
        # keccak_pad goes from one to two blocks at 136: every nonce
        # length's state has leaves on both sides and on the boundary
        for want in (135, 136, 137):
            assert lens[want] > 0, (nl, want, sorted(lens))
    assert {0, 0x7F, 0x80, (1 << 64) - 1} <= \
        {n for nl in range(9) for n in rc.nonces_of_len(nl)}
    assert min(all_lens) < 110 and max(all_lens) > 140


def test_single_account_states_hit_135_to_137_in_both_forms():
    root_form, subtree_form = set(), set()
    for total, accounts in rc.single_account_states():
        (key, (n, b, ch, _)), = accounts
        item = (pyref.nibbles_of(key),
                pyref.account_value(n, b, pyref.EMPTY_ROOT_HASH, ch))
        assert len(pyref._build([item], 0)) == total
        root_form.add(total)
        # the subtree child reference embeds the leaf below the top nibble
        subtree_form.add(len(pyref._build([item], 1)))
    assert {135, 136, 137} <= root_form
    assert {135, 136, 137} <= subtree_form


def test_branch_length_tries_hit_every_target():
    tries = rc.branch_length_tries()
    by_len = {}   # branch RLP length -> set of member counts
    ext_over_branch = 0
    for name, share, k, total, inline_only in rc.BRANCH_TARGETS:
        nodes = list(pyref.storage_nodes(tries[name]))
        kinds = [kind for _, kind, _, _ in nodes]
        assert kinds[:2] == ["ext", "branch"], name  # extension wrap runs
        depth, _, nmem, rlp = nodes[1]
        assert (depth, nmem, len(rlp)) == (share, k, total), name
        kids = [len(r) for _, kind, _, r in nodes[2:] if kind == "leaf"]
        assert len(kids) == k
        if inline_only:
            assert max(kids) < 32, name
        by_len.setdefault(total, set()).add(nmem)
        ext_over_branch += 1
    for want in [31, 32, 33, 56, 58, 135, 136, 137, 257, 259, 271, 272,
                 273, 407, 408, 409, 532]:
        assert want in by_len, want
    # payload 55/56 and 255/256 are totals 56/58 and 257/259
    for want in (135, 136, 137):
        assert any(4 <= m <= 7 for m in by_len[want]), want
        assert any(m >= 12 for m in by_len[want]), want
    # all-inline fans: many members, one keccak block
    assert by_len[115] == {16} and by_len[91] == {12} and by_len[30] == {2}
    assert ext_over_branch == len(rc.BRANCH_TARGETS) == 23


def test_branch_length_state_oracle_matches_pyref():
    accounts, labels = rc.branch_length_state()
    assert len(accounts) >= 600 and len(dict(accounts)) == len(accounts)
    acct, st = to_arrays(dict(accounts))
    got = bind.storage_roots(acct, st)
    want = {name: pyref.storage_root(slots)
            for name, slots in rc.branch_length_tries().items()}
    for i, a in enumerate(acct):
        name = labels[bytes(a["key"])]
        assert bytes(got[i]) == want[name], name
    assert len(np.unique(got, axis=0)) == len(want)


def test_pyref_accelerated_changes_speed_not_results():
    # the GPU proof tests take their references inside pyref.accelerated();
    # it must give the plain walker's node lists and leave pyref as it was
    accounts = dict(rc.account_leaf_grid(2)[0][:40])
    accounts.update(dict(rc.branch_length_state(copies=1)[0][:6]))
    keys = sorted(accounts)
    targets = [keys[0], keys[7], keys[-1], bind.keccak256(b"nobody")]
    plain = [pyref.account_proof(accounts, t) for t in targets]
    build, keccak = pyref._build, pyref.keccak256
    with pyref.accelerated(bind.keccak256):
        fast = [pyref.account_proof(accounts, t) for t in targets]
    assert fast == plain
    assert pyref._build is build and pyref.keccak256 is keccak
    ak = next(k for k in keys if accounts[k][3])
    sk = sorted(accounts[ak][3])[0]
    with pyref.accelerated(bind.keccak256):
        fast = pyref.storage_proof(accounts, ak, sk)
    assert fast == pyref.storage_proof(accounts, ak, sk)
    nodes = [rlp for _, _, _, rlp in pyref.storage_nodes(accounts[ak][3])]
    assert pyref.keccak256(nodes[0]) == pyref.storage_root(accounts[ak][3])
    assert all(n in nodes for n in fast[1])
