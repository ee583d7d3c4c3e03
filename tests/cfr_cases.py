"""Constructed endgames for the CFR solver's tests (tests/test_cfr_cpu.py, tests/test_gpu_cfr.py): the cases of
tests/golden/cfr_reference.npz as tables, and a batch of at most 32 tables around them -- the largest forest the capacity
sweep found, the sizes 1/1/1 .. 2/2/2 in several seat orders, every kind of combination led and to be beaten, both follow
forms, all three actors, idle tables and tables outside the domain.  Built from the spec's words alone (cfr_reference's
make_state); nothing here solves anything."""
import numpy as np

import cfr_reference as cr


def vec(cards):
    """rank values 3..17 -> 15 counts"""
    out = [0] * 15
    for c in cards:
        out[c - 3] += 1
    return out


def case_state(oracle, rows, sizes, pool, first, beat, owner, pick=0, scramble=None):
    """the table of initiate_game(sizes, pool, first, beat, owner): sizes by seat (lord, down, up), pool and beat as 15
    counts, first = the seat to move, owner = the seat that played `beat`; the actor's hand is the first mover's hand of
    deal number `pick` (mod the number of deals).  scramble: a numpy Generator that fills the opponents' count bytes with
    noise (the solver must not read them)"""
    role = (first + 1) % 3
    left = [sizes[2], sizes[0], sizes[1]]
    deals = cr.deal(list(sizes), list(pool))
    hand = deals[pick % len(deals)][first]
    recent = {}
    if any(beat):
        recent[(owner + 1) % 3] = oracle.lookup(np.array(list(beat), np.int8))
    fill = None
    if scramble is not None:
        fill = {r: scramble.integers(0, 5, 15) for r in range(3) if r != role}
    return cr.make_state(hand, role, left, cr.DECK - np.array(pool), recent, rows, fill)


def golden_states(oracle, rows, g, pick=0, scramble=None):
    """the tables of the fixture's cases, in its order"""
    return np.stack([case_state(oracle, rows, [int(x) for x in g["sizes"][c]], [int(x) for x in g["pool"][c]], int(g["first"][c]),
                                [int(x) for x in g["beat"][c]], int(g["owner"][c]), pick, scramble) for c in range(len(g["names"]))])


# (name, sizes [lord, down, up], pool cards, first seat, cards to beat, their owner's seat, deal whose hand the actor holds)
EXTRA = [
    ("the largest forest: 4 5 6 7 and both jokers 2/2/2, lord follows up's 3", [2, 2, 2], [4, 5, 6, 7, 16, 17], 0, [3], 2, 17),
    ("a triple with kicker to be beaten, down follows", [1, 4, 1], [5, 9, 9, 9, 11, 6], 1, [4, 4, 4, 3], 0, 4),
    ("the rocket to be beaten, up follows behind a pass", [1, 2, 2], [3, 8, 8, 12, 15], 2, [16, 17], 0, 3),
    ("a triple to be beaten, lord follows", [3, 1, 2], [7, 7, 7, 10, 10, 13], 0, [5, 5, 5], 2, 5),
    ("4/1/1, lord leads", [4, 1, 1], [3, 3, 6, 9, 12, 14], 0, [], 0, 7),
    ("3/2/1, down leads", [3, 2, 1], [4, 8, 8, 11, 11, 15], 1, [], 1, 9),
    ("2/3/1, up follows the down's single", [2, 3, 1], [5, 7, 10, 10, 13, 17], 2, [6], 1, 2),
    ("2/1/3, up leads", [2, 1, 3], [6, 6, 9, 12, 12, 16], 2, [], 2, 11),
]


def batch(oracle, rows, g, scramble=None):
    """-> (states uint8 [T, 11, 16], names): the fixture's cases (the actor holding the hand of a middle deal), EXTRA, then
    two idle tables and four running ones outside the domain"""
    states = [s for s in golden_states(oracle, rows, g, pick=5, scramble=scramble)]
    names = [str(x) for x in g["names"]]
    for name, sizes, pool, first, beat, owner, pick in EXTRA:
        states.append(case_state(oracle, rows, sizes, vec(pool), first, vec(beat), owner, pick, scramble))
        names.append(name)
    base = case_state(oracle, rows, [2, 1, 2], vec([4, 9, 9, 13, 15]), 1, vec([]), 1, 3, scramble)
    done = base.copy()
    done[cr.F_META, cr.M_DONE] = 1
    fresh = base.copy()
    fresh[cr.F_META, cr.M_DEALT] = 0
    seven = case_state(oracle, rows, [2, 1, 2], vec([4, 9, 9, 13, 15]), 1, vec([]), 1, 3, scramble)
    seven[cr.F_HAND0 + 0, 15] = 4                       # up says 4 cards: 7 in all -- not an endgame, no status bit
    zero = base.copy()
    zero[cr.F_HAND0 + 1, 15] = 0                        # the lord says 0 cards
    short = base.copy()
    short[cr.F_TAKEN, 0] -= 1                           # one card more in the pool than in the hands
    short[cr.F_HIST0, 0] -= 1
    alien = base.copy()
    alien[cr.F_HAND0 + 2, :15] = 0
    alien[cr.F_HAND0 + 2, 0] = 1                        # the actor holds a card that was played
    states += [done, fresh, seven, zero, short, alien]
    names += ["idle: done", "idle: not dealt", "outside: 7 cards", "outside: a left of 0", "outside: pool and hands differ",
              "outside: a hand outside the pool"]
    assert len(states) <= 32
    return np.stack(states), names


def taken_above_deck(oracle, rows, scramble=None):
    """-> states uint8 [2, 11, 16]: batch()'s base table, and a copy whose taken row says five 3s (no hand holds a 3) and
    one 5 fewer, so that the pool still counts as many cards as the hands: outside the domain by the negative pool count alone"""
    base = case_state(oracle, rows, [2, 1, 2], vec([4, 9, 9, 13, 15]), 1, vec([]), 1, 3, scramble)
    over = base.copy()
    over[cr.F_TAKEN, 0] += 1
    over[cr.F_TAKEN, 2] -= 1
    assert over[cr.F_TAKEN, 0] == 5 and not base[cr.F_HAND0:cr.F_HAND0 + 3, 0].any()
    return np.stack([base, over])
