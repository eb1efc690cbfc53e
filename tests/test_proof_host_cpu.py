"""reth_amd/csrc/proof_host.h (the host half of sre_account_proof /
sre_storage_proof: Keccak-256, leaf / extension encoders, RLP list parser,
the proof walk and the per-target assembly) against oracle/pyref.py, as a
plain host executable: tests/proof_main.cpp, built with the address and
undefined-behaviour sanitizers. No GPU, nothing loaded into Python. This
file writes the cases as hex lines; proof_main.cpp documents the records."""
import json
import os
import random
import subprocess

from oracle import bind, pyref
from reth_amd import gen
from tests.test_gpu_proof import _dict_of

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "reth_amd", "csrc")
KE = bind.keccak256(b"")


def _hx(b):
    return bytes(b).hex() or "-"


def _key(nibbles):
    return bytes((nibbles[i] << 4) | nibbles[i + 1] for i in range(0, 64, 2))


def _lcp(items, pos):
    first, last = items[0][0], items[-1][0]
    while first[pos] == last[pos]:
        pos += 1
    return pos


def _trace(items, target):
    """Follow target (nibbles) through the trie of items (sorted
    (nibbles, value)). Returns (rows, from, leaf): the captured rows the
    engine would hold for this path — (key0, P, d, branch RLP) per branch,
    root-first — and the leaf the path ends at with the nibble it starts
    at. Where the path ends short of a leaf (inside an extension, at an
    empty slot) the leaf is the first one under the last branch, as the
    engine's neighbour candidate would be: a distractor for the walk."""
    rows, pos = [], 0
    while len(items) > 1:
        d = _lcp(items, pos)
        rows.append((_key(items[0][0]), pos - 1, d, pyref._build(items, d)))
        kids = [it for it in items if it[0][d] == target[d]]
        if target[pos:d] != items[0][0][pos:d] or not kids:
            return rows, d + 1, pyref._build(items[:1], d + 1)
        items, pos = kids, d + 1
    return rows, pos, pyref._build(items, pos)


def _exts(items, pos=0):
    """(key0, P, d, child branch RLP, extension RLP) of every extension."""
    if len(items) == 1:
        return
    d = _lcp(items, pos)
    if d > pos:
        child = pyref._build(items, d)
        ref = child if len(child) < 32 else b"\xa0" + bind.keccak256(child)
        want = pyref.rlp_list_payload(
            pyref.rlp_str(pyref.hp_encode(items[0][0][pos:d], False)) + ref)
        assert want == pyref._build(items, pos)
        yield _key(items[0][0]), pos - 1, d, child, want
    for nib in range(16):
        kids = [it for it in items if it[0][d] == nib]
        if kids:
            yield from _exts(kids, d + 1)


class _Cases:
    def __init__(self):
        self.lines = []
        self.n = dict.fromkeys("KWLSEAX", 0)

    def add(self, op, *fields):
        self.n[op] = self.n.get(op, 0) + 1
        self.lines.append(" ".join([op] + [str(f) for f in fields]))

    def trie(self, items, proofs, leaf_fields, with_exts):
        """One trie: items as for _trace, proofs = [(key, present, nodes)]
        with pyref's node lists, leaf_fields(key) = the record that
        re-encodes a present key's leaf (op, fields before `from`, fields
        after it)."""
        universe = sorted({n for _, _, nodes in proofs for n in nodes})
        random.Random(len(universe)).shuffle(universe)
        root = bind.keccak256(proofs[0][2][0])
        self.add("N")
        for n in universe:
            self.add("U", _hx(n))
            self.add("K", _hx(n), _hx(bind.keccak256(n)))
            self.add("X", _hx(n))
        for key, present, nodes in proofs:
            want = [len(nodes)] + [_hx(n) for n in nodes]
            self.add("W", _hx(root), _hx(key), int(present), *want)
            rows, frm, leaf = _trace(items, pyref.nibbles_of(key))
            flat = [f for k0, P, d, rlp in rows for f in (_hx(k0), P, d, _hx(rlp))]
            self.add("A", _hx(root), _hx(key), int(present), len(rows), *flat,
                     1, _hx(leaf), *want)
            if present:
                if len(leaf) >= 32 or not rows:
                    assert leaf == nodes[-1]
                op, before, after = leaf_fields(key)
                self.add(op, *before, frm, *after, _hx(leaf))
        if with_exts:
            for k0, P, d, child, want in _exts(items):
                self.add("E", _hx(k0), P, d, _hx(child), _hx(want))

    def account_trie(self, accounts, targets, with_exts=False, proofs=None):
        with pyref.accelerated(bind.keccak256):
            sroot = {k: pyref.storage_root(a[3]) for k, a in accounts.items()}
            items = sorted(
                (pyref.nibbles_of(k), pyref.account_value(a[0], a[1], sroot[k], a[2]))
                for k, a in accounts.items())
            if proofs is None:
                proofs = [(k, k in accounts, pyref.account_proof(accounts, k))
                          for k in targets]

            def fields(k):
                nonce, balance, code_hash, _ = accounts[k]
                return "L", [_hx(k)], [nonce, _hx(balance.to_bytes(32, "big")),
                                       _hx(code_hash), _hx(sroot[k])]
            self.trie(items, proofs, fields, with_exts)

    def storage_trie(self, accounts, acct, targets, with_exts=False,
                     proofs=None):
        slots = accounts[acct][3]
        with pyref.accelerated(bind.keccak256):
            items = sorted((pyref.nibbles_of(k), pyref.rlp_int(v))
                           for k, v in slots.items())
            if proofs is None:
                proofs = [(k, k in slots,
                           pyref.storage_proof(accounts, acct, k)[1])
                          for k in targets]

            def fields(k):
                return "S", [_hx(k)], [_hx(slots[k].to_bytes(32, "big"))]
            self.trie(items, proofs, fields, with_exts)


def _golden(c):
    """Trie 1: the 12-account state of tests/golden/proof_vectors.json with
    every committed account and storage row, absent keys included."""
    v = json.load(open(os.path.join(HERE, "golden", "proof_vectors.json")))
    accounts = {}
    for i in range(12):
        k = bind.keccak256(b"acct" + bytes([i]))
        slots = {bind.keccak256(b"slot" + bytes([i, q])): (i + 1) * 100 + q
                 for q in range(i % 4)}
        accounts[k] = (i, 10**15 + i, KE if i % 3 else bind.keccak256(b"c"),
                       slots)
    c.account_trie(accounts, None, proofs=[
        (bytes.fromhex(r["key"]), r["present"],
         [bytes.fromhex(n) for n in r["nodes"]]) for r in v["accounts"]])
    acct = bytes.fromhex(v["storage"][0]["acct"])
    assert all(r["acct"] == acct.hex() for r in v["storage"])
    c.storage_trie(accounts, acct, None, proofs=[
        (bytes.fromhex(r["slot"]), r["present"],
         [bytes.fromhex(n) for n in r["nodes"]]) for r in v["storage"]])
    return len(v["accounts"]) + len(v["storage"])


def _generated(c):
    """Trie 2: 800 generated accounts; the root is a full 16-child branch
    of 532 bytes (the parser's long list header)."""
    acct, st = gen.gen_state_numpy(800, 3, bind.keccak256_batch)
    accounts = _dict_of(acct, st)
    keys = sorted(accounts)
    targets = [keys[0], keys[100], keys[-1]] + [
        bind.keccak256(b"nope" + bytes([i])) for i in range(5)]
    c.account_trie(accounts, targets)
    assert any(ln.startswith("U f90211") and len(ln) == 2 + 2 * 532
               for ln in c.lines)
    return len(targets)


def _crafted(c):
    """Trie 3: account keys that force extension nodes. Three dicts, since
    an extension at the root needs every key of the trie under it."""
    big = 2**255 + 12345  # 32-byte balance
    n_targets = 0
    # a) two keys equal in their first 31 bytes: 62-nibble (even) root ext
    base = bind.keccak256(b"pair")[:31]
    two = {base + b"\x10": (0, big, KE, {}), base + b"\x70": (7, 0, KE, {})}
    targets = sorted(two) + [
        base[:1] + bytes([base[1] ^ 0x10]) + base[2:] + b"\x10",  # inside ext
        base + b"\x50",  # empty slot of the branch at nibble 62
        base + b"\x13",  # the leaf's last nibble
    ]
    c.account_trie(two, targets, with_exts=True)
    n_targets += len(targets)
    # b) every key shares exactly 5 nibbles: odd root ext; under its branch
    # three lone leaves and a pair sharing 4 more nibbles (an even ext
    # below a branch)
    pre = bytes([0xAB, 0xCD])

    def k5(n5, rest):  # nibbles ab cd e | n5 | rest
        return pre + bytes([0xE0 | n5]) + bind.keccak256(rest)[:29]
    group = {k5(1, b"a"): (0, 1, KE, {}), k5(4, b"b"): (1, big, KE, {}),
             k5(9, b"c"): (2, 2**64, bind.keccak256(b"code"), {})}
    deep = pre + bytes([0xEC, 0x55]) + bind.keccak256(b"deep")[:28]
    group[deep[:31] + b"\x01"] = (3, 5, KE, {})
    group[deep[:5] + bytes([deep[5] ^ 0x80]) + deep[6:31] + b"\x02"] = (4, 6, KE, {})
    lone = k5(1, b"a")
    targets = sorted(group) + [
        pre[:1] + bytes([0xC0]) + lone[2:],            # inside the root ext
        pre + bytes([0xE7]) + lone[3:],                # empty branch slot
        lone[:20] + bytes([lone[20] ^ 1]) + lone[21:],  # at a leaf's path
        deep[:4] + bytes([deep[4] ^ 0x01]) + deep[5:],  # inside the inner ext
    ]
    c.account_trie(group, targets, with_exts=True)
    n_targets += len(targets)
    # c) one key: the leaf is the root
    only = bind.keccak256(b"only")
    targets = [only, bind.keccak256(b"other")]
    c.account_trie({only: (0, big, KE, {})}, targets, with_exts=True)
    return n_targets + len(targets)


def _storage(c):
    """Trie 4: one account with 60 slots valued 1..60 plus the value edges
    0x7f (bare byte), 0x80 and 2**256 - 1; and a second account whose two
    slots share 63 nibbles, so the root extension's child branch (two 3-byte
    leaves) is inline."""
    slots = {bind.keccak256(bytes([i])): i + 1 for i in range(60)}
    edges = {bind.keccak256(b"v" + bytes([i])): v
             for i, v in enumerate([0x7F, 0x80, 2**256 - 1])}
    slots.update(edges)
    acct, tiny = bind.keccak256(b"x"), bind.keccak256(b"tiny")
    twin = bind.keccak256(b"twin")[:31]
    accounts = {acct: (0, 1, KE, slots),
                tiny: (0, 1, KE, {twin + b"\x31": 1, twin + b"\x3a": 2})}
    targets = sorted(slots)[::17] + sorted(edges) + [
        bind.keccak256(b"noslot" + bytes([i])) for i in range(3)]
    c.storage_trie(accounts, acct, targets, with_exts=True)
    n = c.n["E"]
    t2 = sorted(accounts[tiny][3]) + [twin + b"\x35", bind.keccak256(b"far")]
    c.storage_trie(accounts, tiny, t2, with_exts=True)
    assert c.n["E"] == n + 1  # the extension over the inline branch
    return len(targets) + len(t2)


def test_proof_host_matches_pyref(tmp_path):
    c = _Cases()
    n_targets = _golden(c) + _generated(c) + _crafted(c) + _storage(c)
    # padding and block edges of the sponge (rate 136)
    for ln in (0, 135, 136, 137, 272):
        msg = bytes((7 * i + ln) & 0xFF for i in range(ln))
        c.add("K", _hx(msg), _hx(bind.keccak256(msg)))
    # two-item nodes without a hex-prefix flag byte: the path item is a
    # list, or empty
    for node in ("c2c001", "c28001"):
        c.add("M", node, _hx(KE))
    cases = tmp_path / "proof_cases.txt"
    cases.write_text("\n".join(c.lines) + "\n")

    exe = str(tmp_path / "proof_check")
    r = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(HERE, "proof_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checked, failed = (int(x) for x in r.stdout.split()[1::2])
    # per universe node: its hash and 3 parses; per target: the walk and 3
    # assemblies; per present target: its leaf; per extension: its bytes;
    # the 5 sponge edges and the 2 malformed nodes
    nodes = c.n["U"]
    present = c.n["L"] + c.n["S"]
    assert c.n["W"] == c.n["A"] == n_targets and present and c.n["E"] >= 4
    assert failed == 0 and checked == (
        nodes + 5 + 3 * nodes + n_targets + 3 * n_targets + present
        + c.n["E"] + 2), r.stdout
