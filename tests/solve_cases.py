"""Constructed endgames for the exact solver's tests (tests/test_solve_cpu.py, tests/test_gpu_solve.py), built from the words of
solve spec v1 alone: hand-checkable wins and losses, every kind of combination led and to be beaten, both
follow forms, all three actors, idle tables, tables outside the domain -- and the rollout positions the solver was sized on.
Nothing here solves anything.  Cards are rank values 3 .. 17 (16 = black joker, 17 = coloured joker); roles 0 up / 1 lord /
2 down, the turn goes lord -> down -> up."""
import numpy as np

ROW, NFIELDS = 16, 11
F_HAND0, F_HIST0, F_RECENT0, F_TAKEN, F_META = 0, 3, 6, 9, 10
M_ROLE, M_DONE, M_DEALT = 0, 1, 6
DECK = np.array([4] * 13 + [1, 1], np.int64)
UP, LORD, DOWN = 0, 1, 2


def vec(cards):
    out = [0] * 15
    for c in cards:
        out[c - 3] += 1
    return out


def make_state(oracle, info, hands, actor, recent=None):
    """a running table uint8 [11, 16]: hands {role: cards} in the three hand rows (byte 15 = their sizes), recent {role:
    cards} with the category byte, taken = the deck without the hands (so the table is inside the hidden-hand domain too)"""
    s = np.zeros((NFIELDS, ROW), np.uint8)
    held = np.zeros(15, np.int64)
    for r in range(3):
        v = np.array(vec(hands[r]))
        s[F_HAND0 + r, :15], s[F_HAND0 + r, 15] = v, v.sum()
        held += v
    taken = DECK - held
    assert (taken >= 0).all()
    s[F_TAKEN, :15] = taken
    s[F_HIST0, :15] = taken                 # (the histories are not read by the solver; a payload's taken row is their sum)
    for r, cards in (recent or {}).items():
        v = np.array(vec(cards), np.int8)
        aid = oracle.lookup(v)
        assert aid > 0 and (taken >= v).all(), "the combination to beat was played"
        s[F_RECENT0 + r, :15], s[F_RECENT0 + r, 15] = v, info[aid, 0]
    s[F_META, M_ROLE], s[F_META, 2], s[F_META, M_DEALT] = actor, 0xFF, 1
    return s


# (name, up's cards, the lord's, down's, the actor, recent {role: cards}, expected wins per root move or None)
CASES = [
    # ---- hand-checkable
    ("a one-move win: the lord leads its last card", [3], [5], [4], LORD, {}, [1]),
    ("a forced loss: whatever the lord leads, down's 5 beats it and is down's last card", [6, 6], [3, 4], [5], LORD, {}, [0, 0]),
    ("a win only through the right lead: the pair holds the lead, a single loses it", [7], [3, 3, 4], [5], LORD, {}, [0, 0, 1]),
    ("a farmer wins for the partner: down leads low, up's last card goes out", [4], [5, 5, 6], [3, 17], DOWN, {}, [1, 1]),
    ("the partner's win counts behind the lord's pass: up passes, down goes out", [3, 9], [8, 12], [10], UP, {LORD: [8]}, None),
    ("the lord loses to a farmer that is not the actor", [15], [3, 3, 3, 4], [4, 5], DOWN, {}, None),
    # ---- every kind led
    ("leads of one rank: single, pair, triple, bomb", [9], [5, 5, 5, 5, 3], [10], LORD, {}, None),
    ("the rocket led", [9, 9], [16, 17, 3], [10, 4], LORD, {}, None),
    ("a lead with a planner tail: a straight", [8], [3, 4, 5, 6, 7, 9], [10], LORD, {}, None),
    ("a lead with a planner tail: a plane with kickers, a triple line, triples with kickers", [7], [3, 3, 3, 4, 4, 4, 5, 6], [8], LORD, {}, None),
    ("a double line and triples with a pair led by down", [11], [12, 12], [3, 3, 4, 4, 5, 5, 5], DOWN, {}, None),
    ("four with two led by up", [6, 6, 6, 6, 3, 4, 4], [12], [13], UP, {}, None),
    ("a plane with pairs led", [11], [3, 3, 3, 4, 4, 4, 5, 5, 6, 6], [12], LORD, {}, None),
    ("four with two pairs led by down", [12], [13], [6, 6, 6, 6, 3, 3, 4, 4], DOWN, {}, None),
    # ---- every kind to be beaten (the actor follows the previous player's combination)
    ("a single to beat", [8, 5], [9, 9, 3], [10, 4], LORD, {UP: [7]}, None),
    ("a pair to beat", [5, 10], [8, 8, 4], [9, 9, 3], LORD, {UP: [6, 6]}, None),
    ("a triple to beat", [4], [7, 7, 7, 3], [9, 9, 9], LORD, {UP: [5, 5, 5]}, None),
    ("a bomb to beat: a higher bomb, then the rocket", [5], [8, 8, 8, 8, 3], [16, 17, 4], LORD, {UP: [6, 6, 6, 6]}, None),
    ("a triple with kicker to beat, and again: a follow with a tail", [10], [7, 7, 7, 4], [8, 8, 8, 6], LORD, {UP: [5, 5, 5, 3]}, None),
    ("a triple with pair to beat", [10, 10], [4], [6, 6, 6, 9, 9], DOWN, {LORD: [5, 5, 5, 3, 3]}, None),
    ("a straight to beat", [6, 7, 8, 9, 10, 12], [3], [4, 4], UP, {DOWN: [3, 4, 5, 6, 7]}, None),
    ("a double line to beat", [10], [6, 6, 7, 7, 8, 8, 3], [9], LORD, {UP: [3, 3, 4, 4, 5, 5]}, None),
    ("a triple line to beat", [8], [7], [5, 5, 5, 6, 6, 6, 9], DOWN, {LORD: [3, 3, 3, 4, 4, 4]}, None),
    ("a plane with single kickers to beat", [11], [7, 7, 7, 8, 8, 8, 9, 10], [12], LORD, {UP: [3, 3, 3, 4, 4, 4, 5, 6]}, None),
    ("a plane with pairs to beat", [11], [7, 7, 7, 8, 8, 8, 9, 9, 10, 10], [12], LORD, {UP: [3, 3, 3, 4, 4, 4, 5, 5, 6, 6]}, None),
    ("the rocket to beat: nothing but the pass", [6], [3, 4], [5], LORD, {UP: [16, 17]}, [0]),
    ("four with two singles to beat", [3], [7, 7, 7, 7, 8, 9], [4], LORD, {UP: [5, 5, 5, 5, 3, 4]}, None),
    ("four with two pairs to beat", [11], [6, 6, 6, 6, 9, 9, 10, 10], [12], LORD, {UP: [5, 5, 5, 5, 3, 3, 4, 4]}, None),
    # ---- passes
    ("one pass since the combination: the actor's pass hands the lead back to the lord, whose lead down beats", [3], [4, 5], [10], UP, {LORD: [9]}, [1]),
    ("one pass since: down answers the up's pair behind the lord's pass", [7, 8], [12], [9, 9, 3], DOWN, {UP: [6, 6]}, None),
    # ---- the table
    ("transpositions: singles that can go out in many orders", [14, 15], [3, 4, 10, 11], [12, 13], LORD, {}, None),
    ("more positions than a table of 16 holds", [3, 6, 9], [4, 7, 10], [5, 8, 11], LORD, {}, None),
    ("a long proof for a tiny budget", [5, 5, 9], [3, 3, 7, 11, 15], [4, 4, 8, 12], LORD, {}, None),
]


def batch(oracle):
    """-> (states uint8 [T, 11, 16], names, expected): CASES, then two idle tables, one above 12 cards and one whose taken
    row is a card short (outside the hidden form's domain; the open form does not read it)"""
    info = oracle.action_table()[1]
    states = [make_state(oracle, info, {UP: u, LORD: l, DOWN: d}, actor, recent) for _, u, l, d, actor, recent, _ in CASES]
    names = [c[0] for c in CASES]
    expected = [c[6] for c in CASES]
    base = states[2]
    done, fresh = base.copy(), base.copy()
    done[F_META, M_DONE] = 1
    fresh[F_META, M_DEALT] = 0
    big = make_state(oracle, info, {UP: [3, 5, 7, 9, 11], LORD: [4, 6, 8, 10, 12], DOWN: [13, 14, 15]}, LORD)
    short = base.copy()
    short[F_TAKEN, 10] -= 1
    short[F_HIST0, 10] -= 1
    states += [done, fresh, big, short]
    names += ["idle: done", "idle: not dealt", "outside: 13 cards", "outside the hidden form: pool and hands differ"]
    expected += [None] * 4
    assert len(states) <= 40
    return np.stack(states), names, expected


def scrambled(states, rng):
    """copies whose count bytes of the two opponents' hand rows are noise (byte 15, their sizes, stays): what the hidden form
    must not read"""
    out = np.array(states, np.uint8).copy()
    for s in out:
        role = int(s[F_META, M_ROLE]) % 3
        for r in ((role + 1) % 3, (role + 2) % 3):
            s[F_HAND0 + r, :15] = rng.integers(0, 5, 15)
    return out


def jk_states(oracle):
    """tables whose lists differ under the joker-kicker rule set: four with the two jokers as kickers, led and to beat"""
    info = oracle.action_table()[1]
    return np.stack([
        make_state(oracle, info, {UP: [3], LORD: [5, 5, 5, 5, 16, 17, 4], DOWN: [6]}, LORD),
        make_state(oracle, info, {UP: [8], LORD: [7, 7, 7, 7, 16, 17], DOWN: [9]}, LORD, {UP: [5, 5, 5, 5, 3, 4]}),
    ])


_rollouts = {}


def rollout_positions(oracle, max_cards, tables=48, seed=7):
    """the first running state of each of `tables` seed-`seed` random rollouts (the oracle's STEP_RANDOM, no auto-reset) whose
    three hands together hold at most max_cards cards -> uint8 [P, 11, 16]: of 48 rollouts 32 get to 9 cards or fewer before
    they end and 44 to 12 or fewer"""
    k = (oracle.num_actions(), max_cards, tables, seed)
    if k not in _rollouts:
        env = oracle.OracleEnv(tables, seed=seed)
        env.reset()
        st = env.state.reshape(tables, NFIELDS, ROW)
        found = {}
        for _ in range(200):
            cards = st[:, F_HAND0:F_HAND0 + 3, :15].astype(np.int64).sum((1, 2))
            for t in np.flatnonzero((st[:, F_META, M_DONE] == 0) & (cards <= max_cards)):
                found.setdefault(int(t), st[t].copy())
            if (st[:, F_META, M_DONE] == 1).all():
                break
            env.legal()
            env.step(0, auto_reset=False)
        _rollouts[k] = np.stack([found[t] for t in sorted(found)])
    return _rollouts[k]
