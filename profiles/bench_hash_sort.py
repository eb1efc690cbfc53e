"""Plain rows -> resident sorted hashed state, two ways, on one GPU:

  (a) engine.set_plain_device_tensors: the engine's own key kernels, radix
      sort and gathers (sre_set_plain_state_device);
  (b) the same job with what the tree had before: keccak_batch_device for
      the keys, gen._argsort_keys_t (stable torch.argsort passes over int64
      columns) for the order, torch row gathers for the rows.

The legs alternate: one warm-up each, then --reps timed repetitions of each,
a host clock around calls that end in a synchronise. The roots of the two
results must agree. Writes min / median / spread of both legs and (a)'s
counters as JSON.

  python profiles/bench_hash_sort.py --accounts 2000000 --slots 64 \
      --out profiles/hash_sort_2Mx64.json

HBM: (a) peaks at about input + output + 2 x 12 B/row of pairs + 32 B/row of
hashed slot keys (~150 GB at 10M x 64); (b) holds its own output, two hashed
key arrays and several int64 columns next to the engine's resident copy, so
at 10M x 64 the two legs do not fit a 288 GB device side by side. 2M x 64
does.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from reth_amd import gen, plain  # noqa: E402
from reth_amd.engine import StateRootEngine  # noqa: E402


def leg_a(eng, pa, ps):
    t0 = time.perf_counter()
    eng.set_plain_device_tensors(pa, ps)  # synchronises before returning
    return time.perf_counter() - t0, None


def leg_b(eng, pa, ps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    na, ns = pa.shape[0], ps.shape[0]
    dev = pa.device
    hk = torch.empty((na, 32), dtype=torch.uint8, device=dev)
    eng.keccak_batch_device(pa, 20, hk)  # address = first 20 B of a 96-B row
    order = gen._argsort_keys_t(hk)
    acct = torch.empty((na, 104), dtype=torch.uint8, device=dev)
    acct[:, 0:32] = hk[order]
    acct[:, 32:104] = pa[order, 24:96]
    del order
    ha = torch.empty((ns, 32), dtype=torch.uint8, device=dev)
    eng.keccak_batch_device(ps, 20, ha)
    slots = ps[:, 20:52].contiguous()
    hs = torch.empty((ns, 32), dtype=torch.uint8, device=dev)
    eng.keccak_batch_device(slots, 32, hs)
    del slots
    # stable: slot key minor, then account key major
    order = gen._argsort_keys_t(hs)
    order = order[gen._argsort_keys_t(ha[order])]
    st = torch.empty((ns, 96), dtype=torch.uint8, device=dev)
    st[:, 0:32] = ha[order]
    st[:, 32:64] = hs[order]
    st[:, 64:96] = ps[order, 52:84]
    del order, ha, hs
    torch.cuda.synchronize()
    return time.perf_counter() - t0, (acct, st)


def summary(ts):
    return {"min_ms": min(ts) * 1e3, "median_ms": statistics.median(ts) * 1e3,
            "max_ms": max(ts) * 1e3, "reps_ms": [t * 1e3 for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accounts", type=int, default=10_000_000)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    eng = StateRootEngine(0)
    pa, ps = plain.gen_plain_torch(args.accounts, args.slots, device="cuda")
    # arrival order: accounts shuffled, storage grouped by address
    pa = pa[torch.randperm(pa.shape[0], device="cuda",
                           generator=torch.Generator("cuda").manual_seed(1))
            ].contiguous()
    torch.cuda.synchronize()

    ta, tb = [], []
    root_a = root_b = None
    for rep in range(args.reps + 1):  # rep 0 warms up both legs
        dt, _ = leg_a(eng, pa, ps)
        if rep:
            ta.append(dt)
        else:
            root_a = eng.root()
            counters = eng.hash_sort_counters()
        dt, out = leg_b(eng, pa, ps)
        if rep:
            tb.append(dt)
        else:
            eng.set_device_tensors(*out)
            root_b = eng.root()
            eng.release_borrowed()
        del out
        print(f"rep {rep}: a {ta[-1] * 1e3 if ta else float('nan'):.1f} ms  "
              f"b {tb[-1] * 1e3 if tb else float('nan'):.1f} ms", flush=True)
    assert root_a == root_b, (root_a.hex(), root_b.hex())

    res = {"shape": f"{args.accounts}x{args.slots}",
           "accounts": args.accounts, "storage_rows": int(ps.shape[0]),
           "device": torch.cuda.get_device_name(0),
           "root": root_a.hex(), "roots_agree": True,
           "a_set_plain_device_tensors": summary(ta),
           "b_keccak_batch_torch_argsort_gather": summary(tb),
           "speedup_median": statistics.median(tb) / statistics.median(ta),
           "counters": counters}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
