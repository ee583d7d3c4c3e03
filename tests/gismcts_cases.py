"""The roots tests/test_gismcts_cpu.py and tests/test_gpu_gismcts.py search (search spec v4, guided ISMCTS): the
seven tables of guided_cases.build(hidden=True) -- three small endings, a mid-game root with a list beyond a 64-lane round, a
table never dealt, a done one, and one outside the hidden-hand domain -- at guided_cases' budget, trees, salts and roles
mask (up, table 5, is left out).  The endings' opponents hold two or three cards each out of a pool of four to six, so the
worlds of the iterations differ and one tree meets lists that lack a child's move and lists that offer new ones.
  7  one more ending, the lord leads a single and a pair against two cards each of four ranks above them: with the hashed
     evaluator its trees meet, in both modes, two selectable siblings of one value (equal V, W and availability count), which
     the seven do only in the `sides` mode -- a node's children are made on different visits, so their counts differ unless
     the worlds left the older one's move out exactly as often"""
import numpy as np

import constructed_states as cs
import guided_cases as gc
import playout_hidden_cases as hc

SEED, GID_BASE = gc.SEED, gc.GID_BASE
BUDGET, TREES, SALTS = gc.BUDGET, gc.TREES, gc.SALTS
ROLES = gc.ROLES_HIDDEN
MID, NOT_DEALT, DONE, MASKED, OUTSIDE = gc.MID, gc.NOT_DEALT, gc.DONE, gc.MASKED, gc.OUTSIDE
TIES = 7
LIVE = (0, 1, MID, TIES)


def build(oracle, table):
    """states uint8 [8, 11, 16]"""
    ties = hc._table({3: 1, 2: 2}, {7: 1, 6: 1}, {5: 1, 4: 1}, role=1)
    cs.check_consistent(ties, table)
    return np.concatenate([gc.build(oracle, table, hidden=True), ties])


def coverage(items, budget):
    """what the traces of gismcts_reference.gismcts(trace=True) walked through, by name: every entry must be true for the exact
    comparison on these roots to mean what it says"""
    iters = [r for it in items for r in it.iters]
    sels = [s for r in iters for s in r["sel"]]
    return {
        "a terminal child at expansion": any(r["expand"] is not None and not r["pending"] and r["winner"] >= 0 for r in iters),
        "a terminal node reached by selection": any(r["terminal"] for r in iters),
        "a pending leaf on the root's side": any(r["pending"] and r["own"] for r in iters),
        "a pending leaf on the other side": any(r["pending"] and not r["own"] for r in iters),
        "a clamped value at each end": any(r["value"] == 0 for r in iters) and any(r["value"] == 1024 for r in iters),
        "a selection tie broken by index": any(tied and j == int(np.flatnonzero(v == v[j])[0]) for (_, _, j, _, tied, v, _) in sels),
        "a minimum step": any(not mx for (_, _, _, mx, _, _, _) in sels),
        "a selection below the root": any(depth >= 1 for (depth, _, _, _, _, _, _) in sels),
        "an expansion index >= 64 in a list > 64": any(r["expand"] is not None and r["expand"][2] > 64 and r["expand"][1] >= 64
                                                       for r in iters),
        "the last iteration's leaf is backed up by close": any(it.iters[budget - 1]["pending"] for it in items),
        "an existing child's move is not in this world's list": any(r["missing"] for r in iters),
        "an expansion at a node an earlier world found fully expanded": any(r["expand"] is not None and r["expand"][4] for r in iters),
        "a selection among fewer children than the node owns": any(len(v) < owned for (_, _, _, _, _, v, owned) in sels),
    }
