"""The roots tests/test_guided_cpu.py and tests/test_gpu_guided.py search (search spec v3), built with
constructed_states: small enough that a 96-iteration tree meets terminal nodes again, and one list beyond a 64-lane round.
  0  ending, the lord leads: a pair and a single against two cards each (7 cards)
  1  ending, down (a farmer) leads, its partner up moves next (7 cards): the two modes part, both sides own pending leaves
  2  mid-game: a deal advanced by the random policy to a root whose list has 65 .. 90 moves (budget 96 expands it fully)
  3  never dealt          4  done (a one-card lord after its only move)
  5  ending, up leads (6 cards): the table a `roles` mask without up leaves out
  6  hidden form only: a running table outside the hidden-hand domain (status bit 6)"""
import numpy as np

import constructed_states as cs
import playout_hidden_cases as hc

SEED, GID_BASE = 17, 2 ** 32 + 4242       # table_id_base above 2^32: the high word of the RNG counter is in play
BUDGET, TREES = 96, 2
SALTS = (0, 5)
ROLES_HIDDEN = 0b110                      # up (role 0) is left out
MID, NOT_DEALT, DONE, MASKED, OUTSIDE = 2, 3, 4, 5, 6


def mid_game(oracle, lo=65, hi=90):
    """the first table of a few deals whose actor's list has lo .. hi moves after 0 .. 8 random plies"""
    n = 24
    plies = np.arange(n) % 9
    ref = oracle.OracleEnv(n, seed=SEED, gid_base=GID_BASE)
    ref.reset()
    for it in range(int(plies.max())):
        ref.legal()
        ref.step(oracle.STEP_IDS, np.where(plies > it, -1, -2).astype(np.int32), auto_reset=False)   # -1 random, -2 no move
    off, _, _ = ref.legal()
    size = np.diff(off)
    st = ref.state.reshape(n, 11, 16).copy()
    ok = np.flatnonzero((size >= lo) & (size <= hi) & cs.running(st))
    assert len(ok), "no root with a list of %d .. %d moves among the deals" % (lo, hi)
    return st[ok[0]:ok[0] + 1]


def build(oracle, table, hidden=False):
    """states uint8 [6 or 7, 11, 16]"""
    lord = hc._table({0: 2, 4: 1}, {1: 1, 5: 1}, {2: 1, 6: 1}, role=1)
    down = hc._table({0: 1, 3: 1}, {1: 1, 5: 1}, {2: 1, 4: 1, 6: 1}, role=2)
    up = hc._table({1: 1, 7: 1}, {0: 1, 9: 1}, {3: 1, 8: 1}, role=0)
    one = hc._table({4: 1}, {0: 2, 1: 1}, {2: 1, 3: 2}, role=1)
    done = cs.step(one, table, [1 + 4])
    assert done[0, cs.F_META, cs.M_DONE] == 1
    states = [lord, down, mid_game(oracle), np.zeros_like(lord), done, up]
    if hidden:
        states.append(hc.out_of_domain()[1][:1])
    states = np.concatenate(states)
    cs.check_consistent(states[[0, 1, 2, 4, 5]], table)
    return states


def coverage(items, budget):
    """what the traces of guided_reference.guided(trace=True) walked through, by name: every entry must be true for the exact
    comparison on these roots to mean what it says"""
    iters = [r for it in items for r in it.iters]
    sels = [s for r in iters for s in r["sel"]]
    return {
        "a terminal child at expansion": any(r["expand"] is not None and not r["pending"] and r["winner"] >= 0 for r in iters),
        "a terminal node reached by selection": any(r["terminal"] for r in iters),
        "a pending leaf on the root's side": any(r["pending"] and r["own"] for r in iters),
        "a pending leaf on the other side": any(r["pending"] and not r["own"] for r in iters),
        "a clamped value at each end": any(r["value"] == 0 for r in iters) and any(r["value"] == 1024 for r in iters),
        "a selection tie broken by index": any(tied and j == int(np.flatnonzero(v == v[j])[0]) for (_, _, j, _, tied, v) in sels),
        "a minimum step": any(not mx for (_, _, _, mx, _, _) in sels),
        "a selection below the root": any(depth >= 1 for (depth, _, _, _, _, _) in sels),
        "a list beyond one 64-lane round": any(r["expand"] is not None and r["expand"][2] > 64 and r["expand"][1] >= 64 for r in iters),
        "the last iteration's leaf is backed up by close": any(it.iters[budget - 1]["pending"] for it in items),
    }
