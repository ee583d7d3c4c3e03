"""States for the hidden-hand playouts (playout spec v2), shared by tests/test_playout_hidden_cpu.py and
tests/test_gpu_playout_hidden.py.  Every rng stream is fixed; nothing here touches the GPU library.
  game_states   37 tables from reset(): table i is a fresh deal advanced by DEPTH[i % 3] + (i // 3) % 3 random plies --
                depths 0, 12 and 30 with one and two plies more, so that each depth is seen by all three actor roles
  degenerate    imported pools at the edges of the redeal: one card left with an opponent, both jokers unseen, all four
                copies of a rank unseen (and the three at once)
  out_of_domain imported states the kernel must refuse, one per violation"""
import numpy as np

import constructed_states as cs
import playout_hidden_reference as phr

SEED, GID_BASE = 9, 2 ** 33 + 1000          # table_id_base above 2^32: the high word of the RNG counter is in play
N_GAMES = 37
DEPTH = (0, 12, 30)


def plies_of(i):
    return DEPTH[i % 3] + (i // 3) % 3


def game_states(oracle, seed=SEED, gid_base=GID_BASE, n=N_GAMES):
    plies = np.array([plies_of(i) for i in range(n)])
    ref = oracle.OracleEnv(n, seed=seed, gid_base=gid_base)
    ref.reset()
    for it in range(int(plies.max())):
        ref.legal()
        ref.step(oracle.STEP_IDS, np.where(plies > it, -1, -2).astype(np.int32), auto_reset=False)   # -1 random, -2 no move
    return ref.state.reshape(n, 11, 16).copy()


def _table(hand, nxt, prv, role, ply=7):
    """one consistent running table from three hands {rank: count}; what nobody holds was played by the previous player"""
    h = np.zeros((1, 3, 15), np.int64)
    for r, cards in ((role, hand), ((role + 1) % 3, nxt), ((role + 2) % 3, prv)):
        for rank, c in cards.items():
            h[0, r, rank] = c
    hist = np.zeros((1, 3, 15), np.int64)
    hist[0, (role + 2) % 3] = cs.DECK - h[0].sum(0)
    assert (hist >= 0).all()
    return cs.pack_state(h, hist, role=role, ply=ply)


def degenerate():
    """(names, states uint8 [n, 11, 16]): every recent row empty (the actor leads)"""
    cases = {
        "one card left with the next player": _table({0: 2, 5: 1}, {3: 1}, {3: 1, 4: 2, 9: 1}, role=1),
        "one card left with the previous player": _table({1: 1, 2: 1}, {6: 3, 7: 1}, {8: 1}, role=0),
        "one card each": _table({4: 1}, {13: 1}, {14: 1}, role=2),
        "both jokers unseen": _table({0: 1, 1: 1, 2: 2}, {13: 1, 5: 1}, {14: 1, 5: 2, 6: 1}, role=1),
        "four of a rank unseen": _table({3: 2, 12: 1}, {7: 3, 1: 1}, {7: 1, 2: 2}, role=2),
        "jokers and four of a rank and a single card": _table({10: 1, 11: 1}, {13: 1}, {14: 1, 9: 4, 0: 1}, role=0),
        # (the actor's list has a row more under the joker-kicker rule set: the two builds differ on this root)
        "the actor holds four of a rank and both jokers": _table({2: 4, 13: 1, 14: 1, 0: 1}, {5: 2, 6: 1}, {5: 1, 7: 2}, role=1),
    }
    return list(cases), np.concatenate(list(cases.values()))


def out_of_domain():
    """(names, states): running tables outside the domain of spec v2, each by one violation"""
    base = _table({0: 2, 5: 1}, {3: 2, 6: 1}, {3: 1, 4: 2, 9: 1}, role=1)

    def variant(f):
        s = base.copy()
        f(s[0])
        return s

    def more_taken(s):
        s[cs.F_TAKEN, 5] = 4                      # hand 1 + taken 4 > 4 copies: unseen_5 = -1

    def joker_twice(s):
        s[cs.F_TAKEN, 13] = 2                     # unseen_13 = -1

    def sum_low(s):
        s[cs.F_HAND0 + 2, 15] -= 1                # sum unseen = n_next + n_prev + 1

    def sum_high(s):
        s[cs.F_HAND0 + 0, 15] += 1

    def next_empty(s):
        s[cs.F_HAND0 + 0, 15] += s[cs.F_HAND0 + 2, 15]
        s[cs.F_HAND0 + 2, 15] = 0                 # the sizes still add up, n_next = 0

    def prev_empty(s):
        s[cs.F_HAND0 + 2, 15] += s[cs.F_HAND0 + 0, 15]
        s[cs.F_HAND0 + 0, 15] = 0

    cases = {"a negative unseen count": more_taken, "a joker taken twice": joker_twice, "sizes one short": sum_low,
             "sizes one over": sum_high, "next player's size 0": next_empty, "previous player's size 0": prev_empty}
    return list(cases), np.concatenate([variant(f) for f in cases.values()])


def strip_opponents(states, fill=0):
    """copies whose opponents' 15 count bytes are `fill` (a value, or an rng for noise); byte 15 stays"""
    s = np.array(states, np.uint8).copy()
    for t in range(len(s)):
        role = int(s[t, cs.F_META, cs.M_ROLE]) % 3
        for r in ((role + 1) % 3, (role + 2) % 3):
            s[t, r, :15] = fill.integers(0, 256, 15) if hasattr(fill, "integers") else fill
    return s


def true_worlds(states, K):
    """(out, took_part, out_of_domain) in the shape of phr.worlds() with every world = the hands the opponents really hold"""
    s = np.asarray(states, np.uint8)
    W = np.zeros((len(s), K, 2, 16), np.uint8)
    for t in range(len(s)):
        role = int(s[t, cs.F_META, cs.M_ROLE]) % 3
        W[t, :, 0], W[t, :, 1] = s[t, (role + 1) % 3], s[t, (role + 2) % 3]
    return W, cs.running(s), np.zeros(len(s), bool)
