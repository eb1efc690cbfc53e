"""What revert capture and unwind cost on one GPU.

A state of --accounts x --slots is generated on the device, one account with
--big-slots slots is added to it, and the result S0 is retained once. Two
deltas are then timed from S0, each followed by its way back, so that every
repetition starts from the same arrays:

  dirty  the delta shape of `bench.py --incremental --dirty
         --incremental-slots N`: --delta-accounts account rows (4/5 modified,
         1/10 inserted, 1/10 destroyed) and 4 fresh slots per modified
         account;
  big    one account row that destroys the --big-slots account: the revert
         copies that whole segment.

Per delta and repetition, alternating:

  off         incremental_root(delta), capture off
  back_host   incremental_root(revert rows kept on the host), capture off;
              the way back a caller without unwind() takes
  on          incremental_root(delta), capture on
  unwind      unwind(), capture on (so it captures the redo as well)

A host clock around calls that end in a synchronise (every one of these
ends in a blocking copy of the root). The roots of S0 and of the post state
must come out the same in every repetition. Writes min / median / spread of
every leg and the revert counters as JSON.

  python profiles/bench_reverts.py --accounts 2000000 --slots 64 \
      --out profiles/reverts_2Mx64.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from reth_amd import gen  # noqa: E402
from reth_amd.engine import (DELTA_DTYPE, STORAGE_DTYPE,  # noqa: E402
                             StateRootEngine)

KE = np.frombuffer(bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653"
                                 "ca82273b7bfad8045d85a470"), np.uint8)


def keccak_rows(eng, msgs):
    """keccak256 of every row of a (n, len) uint8 array, on the device"""
    t = torch.from_numpy(np.ascontiguousarray(msgs)).cuda()
    out = torch.empty((t.shape[0], 32), dtype=torch.uint8, device="cuda")
    eng.keccak_batch_device(t, t.shape[1], out)
    return out.cpu().numpy()


def counter_msgs(counters, width=8):
    m = np.zeros((len(counters), width), dtype=np.uint8)
    m[:, :8] = np.asarray(counters, dtype="<u8").view(np.uint8).reshape(-1, 8)
    return m


def be_u256(values):
    out = np.zeros((len(values), 32), dtype=np.uint8)
    out[:, 24:] = np.asarray(values, dtype=">u8").view(np.uint8).reshape(-1, 8)
    return out


def key_order(*cols):
    """argsort of rows by the concatenated 32-byte keys in cols (major first)"""
    words = []
    for c in cols:
        w = np.ascontiguousarray(c).view(">u8").reshape(len(c), 4)
        words += [w[:, k] for k in range(4)]
    return np.lexsort(words[::-1])


def dirty_delta(eng, accounts, nd):
    """bench.py's --incremental --dirty --incremental-slots delta"""
    n_mod, n_del = (nd * 4) // 5, nd // 10
    n_new = nd - n_mod - n_del
    counters = np.concatenate([np.arange(n_mod), accounts + np.arange(n_new),
                               n_mod + np.arange(n_del)]).astype(np.uint64)
    keys = keccak_rows(eng, counter_msgs(counters))
    d = np.zeros(nd, dtype=DELTA_DTYPE)
    d["key"] = keys
    d["code_hash"] = KE
    d["nonce"][:n_mod] = counters[:n_mod] & 0xFFFF
    d["balance"][:n_mod] = be_u256(10**18 + counters[:n_mod])
    d["nonce"][n_mod:n_mod + n_new] = 1
    d["balance"][n_mod:n_mod + n_new] = be_u256(
        5 * 10**17 + counters[n_mod:n_mod + n_new])
    d["deleted"][n_mod + n_new:] = 1
    d = d[key_order(d["key"])]
    msgs = counter_msgs(np.repeat(counters[:n_mod], 4), 12)
    msgs[:, 8] = np.tile(np.arange(4, dtype=np.uint8), n_mod)
    msgs[:, 9] = 0xD5
    s = np.zeros(4 * n_mod, dtype=STORAGE_DTYPE)
    s["acct_key"] = np.repeat(keys[:n_mod], 4, axis=0)
    s["slot_key"] = keccak_rows(eng, msgs)
    s["value"] = be_u256(10**9 + 7 * np.repeat(np.arange(n_mod), 4) +
                         np.tile(np.arange(4), n_mod))
    return d, s[key_order(s["acct_key"], s["slot_key"])]


def big_account(eng, n_slots):
    """(delta that inserts one account with n_slots slots, delta that
    destroys it)"""
    key = keccak_rows(eng, np.array([list(b"big-acct")], dtype=np.uint8))[0]
    add = np.zeros(1, dtype=DELTA_DTYPE)
    add["key"], add["nonce"], add["code_hash"] = key, 1, KE
    drop = add.copy()
    drop["nonce"], drop["deleted"] = 0, 1
    msgs = counter_msgs(np.arange(n_slots, dtype=np.uint64), 12)
    msgs[:, 9] = 0xB1
    s = np.zeros(n_slots, dtype=STORAGE_DTYPE)
    s["acct_key"] = key
    s["slot_key"] = keccak_rows(eng, msgs)
    s["value"] = be_u256(1 + np.arange(n_slots))
    return (add, s[key_order(s["slot_key"])]), \
        (drop, np.zeros(0, dtype=STORAGE_DTYPE))


def timed(fn, *args):
    t0 = time.perf_counter()
    out = fn(*args)  # ends in a blocking copy of the root
    return time.perf_counter() - t0, out


def summary(ts):
    return {"min_ms": min(ts) * 1e3, "median_ms": statistics.median(ts) * 1e3,
            "max_ms": max(ts) * 1e3, "reps_ms": [t * 1e3 for t in ts]}


def run_legs(eng, delta, root0, reps):
    """the four legs from S0 and back, reps + 1 times (the first warms up)"""
    ts = {k: [] for k in ("off", "back_host", "on", "unwind")}
    rev = root1 = counters = None
    for rep in range(reps + 1):
        got = {}
        if rev is not None:
            eng.capture_reverts(False)
            got["off"], r = timed(eng.incremental_root, *delta)
            assert r == root1
            got["back_host"], r = timed(eng.incremental_root, *rev)
            assert r == root0
        eng.capture_reverts(True)
        got["on"], r = timed(eng.incremental_root, *delta)
        assert root1 in (None, r)
        root1 = r
        if rev is None:
            rev, counters = eng.revert(), eng.revert_counters()
        got["unwind"], r = timed(eng.unwind)
        assert r == root0, "unwind did not restore the root"
        eng.capture_reverts(False)
        if rep:
            for k, v in got.items():
                ts[k].append(v)
        print(f"rep {rep}: " + "  ".join(f"{k} {v * 1e3:.2f} ms"
                                         for k, v in got.items()), flush=True)
    res = {k: summary(v) for k, v in ts.items()}
    res["delta_rows"] = [len(delta[0]), len(delta[1])]
    res["revert_rows"] = [len(rev[0]), len(rev[1])]
    res["revert_counters"] = counters
    res["on_minus_off_median_ms"] = \
        res["on"]["median_ms"] - res["off"]["median_ms"]
    res["unwind_over_on_median"] = \
        res["unwind"]["median_ms"] / res["on"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accounts", type=int, default=2_000_000)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--delta-accounts", type=int, default=5000)
    ap.add_argument("--big-slots", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    eng = StateRootEngine(0)
    acct_t, st_t = gen.gen_state_torch(args.accounts, args.slots,
                                       eng.keccak_batch_device, device="cuda")
    torch.cuda.synchronize()
    eng.set_device_tensors(acct_t, st_t)
    torch.cuda.empty_cache()
    dirty = dirty_delta(eng, args.accounts, args.delta_accounts)
    add_big, drop_big = big_account(eng, args.big_slots)

    eng.root_retaining()
    root0 = eng.incremental_root(*add_big)  # S0, engine-owned from here on
    eng.release_borrowed()
    del acct_t, st_t
    torch.cuda.empty_cache()
    na, ns = eng.resident_counts()

    res = {"shape": f"{args.accounts}x{args.slots}+1x{args.big_slots}",
           "accounts": na, "storage_rows": ns,
           "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "root_s0": root0.hex(),
           "dirty": run_legs(eng, dirty, root0, args.reps),
           "big": run_legs(eng, drop_big, root0, args.reps)}
    assert eng.resident_counts() == (na, ns)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
