"""What tests/test_puct_cpu.py and tests/test_gpu_puct.py search (search spec v5): guided_cases' roots, budget,
trees and salts, and a hashed evaluator that hands back a value and a row of prior weights per (row, launch)."""
import numpy as np

import guided_cases as gc
import guided_reference as gr

SEED, GID_BASE, BUDGET, TREES, SALTS, ROLES_HIDDEN = gc.SEED, gc.GID_BASE, gc.BUDGET, gc.TREES, gc.SALTS, gc.ROLES_HIDDEN
MID, NOT_DEALT, DONE, MASKED, OUTSIDE = gc.MID, gc.NOT_DEALT, gc.DONE, gc.MASKED, gc.OUTSIDE
build = gc.build
C = 1.25
STRIDE = 512
SMALL_POOL = 16                # room for one run of at most 16 weights: every other node falls back to uniform


def _fnv(rows, extra):
    rows = np.asarray(rows, np.uint8).reshape(len(rows), -1).astype(np.uint64)
    h = np.full(len(rows), 0xCBF29CE484222325, np.uint64)
    with np.errstate(over="ignore"):
        for b in range(rows.shape[1]):
            h = (h ^ rows[:, b]) * np.uint64(0x100000001B3)
        h = (h ^ np.uint64(extra)) * np.uint64(0x100000001B3)
    return h


def hash_eval(rows, need, i):
    """(values, priors uint8 [len(need), STRIDE]): the value is guided_reference.hash_leaf's (integers in [-50, 1100]: the clamp
    at both ends, equal scores among siblings); the weights are a hash of (row, launch, list index), in one of four manners
    picked by the row's hash: 0 all zero (a uniform node), 1 a single nonzero weight (at an index below 80: beyond a short
    list that is an all-zero run again), 2 multiples of 64 (equal weights: ties), 3.. any byte"""
    values = gr.hash_leaf(rows, need, i)
    h = _fnv(rows, i)
    j = np.arange(STRIDE, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        x = (h[:, None] ^ (j * np.uint64(0x9E3779B97F4A7C15))) * np.uint64(0xD6E8FEB86659FD93)
    x = ((x >> np.uint64(32)) ^ x) >> np.uint64(24)
    fine = (x & np.uint64(0xFF)).astype(np.uint8)
    manner = ((h >> np.uint64(8)) % np.uint64(8)).astype(np.int64)[:, None]
    single = (h >> np.uint64(20)) % np.uint64(80)
    weights = np.where(manner == 0, 0,
                       np.where(manner == 1, np.where(j == single[:, None], 200, 0),
                                np.where(manner == 2, fine & 0xC0, fine))).astype(np.uint8)
    return values, weights


def coverage(items, budget):
    """what the traces of puct_reference.puct(trace=True) walked through, by name"""
    iters = [r for it in items for r in it.iters]
    sels = [s for r in iters for s in r["sel"]]
    return {
        "an unvisited index chosen over visited ones": any(not has and kids > 0 for (_, _, _, has, kids, _, _) in sels),
        "a visited child chosen while unvisited indices remain": any(has and kids < len(v) for (_, _, _, has, kids, _, v) in sels),
        "a tie broken by index": any(tied and j == int(np.flatnonzero(v == v[j])[0]) for (_, _, j, _, _, tied, v) in sels),
        "a terminal child at expansion": any(r["expand"] is not None and not r["pending"] and r["winner"] >= 0 for r in iters),
        "a terminal node reached by selection": any(r["terminal"] for r in iters),
        "a node on the root's side": any(r["pending"] and r["own"] and not r["root"] for r in iters),
        "a node on the other side": any(r["pending"] and not r["own"] for r in iters),
        "a list beyond one 64-lane round, an index >= 64 selected": any(len(v) > 64 and j >= 64 for (_, _, j, _, _, _, v) in sels),
        "an all-zero prior run": any(r["pending"] and r["S"] == 0 for r in iters),
        "a run with a single nonzero weight": any(r["pending"] and r["S"] == 200 for r in iters),
        "the last iteration's leaf is backed up by close": any(it.iters[budget - 1]["pending"] for it in items),
        "a clamped value at each end": any(r["value"] == 0 for r in iters) and any(r["value"] == 1024 for r in iters),
        "iteration 0 evaluates the root": all(it.iters[0]["root"] and it.iters[0]["pending"] and it.iters[0]["moves"] == 0 for it in items),
    }
