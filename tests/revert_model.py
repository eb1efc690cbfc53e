"""The revert of a delta (include/sre.h, "revert capture") on the dict
states of tests/delta_contract.py (CPU-only; no engine import).

`revert_of(pre, delta)` is the definition, one decision per delta row; it
knows keys and values only. The result is a delta in the same
`(rows, strows)` form: applied to the post-delta state it gives `pre` back.
`counts_of` names the four numbers sre_get_revert_counters reports.
"""
from tests import delta_contract as dc

KE = dc.KE


def _walk(accounts, delta):
    rows, strows = delta
    rrows, from_delta, from_wipes, no_row = [], [], [], 0
    inserted = set()
    for k, _n, _b, _ch, dead in rows:
        if k in accounts:
            # upserted or destroyed: the old account row comes back ...
            n, b, ch, slots = accounts[k]
            rrows.append((k, n, b, ch, 0))
            if dead:  # ... and with a destroyed account ALL its storage
                from_wipes += [(k, sk, v) for sk, v in slots.items()]
        elif not dead:
            inserted.add(k)
            rrows.append((k, 0, 0, KE, 1))
        else:
            no_row += 1  # deleting what is not there
    for ak, sk, v in strows:
        if ak in inserted or ak not in accounts:
            # the revert destroys an inserted account, storage included; a
            # row for an unknown account was a no-op deletion
            no_row += 1
        elif sk in accounts[ak][3]:
            from_delta.append((ak, sk, accounts[ak][3][sk]))
        elif v:
            from_delta.append((ak, sk, 0))
        else:
            no_row += 1  # deleting a slot that is not there
    return rrows, from_delta, from_wipes, no_row


def revert_of(accounts, delta):
    """The revert of the VALID `delta` over `accounts`, which stays
    untouched. Account rows in delta order, storage rows sorted."""
    assert dc.verdict(accounts, *delta) is None
    rrows, from_delta, from_wipes, _ = _walk(accounts, delta)
    # a storage row for an account destroyed in the same delta is rejected,
    # so the two sources never share an account
    assert not {r[0] for r in from_delta} & {r[0] for r in from_wipes}
    return rrows, sorted(from_delta + from_wipes)


def counts_of(accounts, delta):
    """engine.revert_counters() of the capture of `delta` over `accounts`"""
    rrows, from_delta, from_wipes, no_row = _walk(accounts, delta)
    return {"acct_rows": len(rrows), "st_rows": len(from_delta),
            "wiped_rows": len(from_wipes), "no_row": no_row}


def normalised(accounts):
    """dict state with list values: util.random_accounts yields tuples and
    delta_contract.apply writes lists"""
    return {k: [v[0], v[1], v[2], dict(v[3])] for k, v in accounts.items()}
