"""Constructed states for the seam inside k_rollout's lists: every list starts with one closed-form round (a lead: the
singles, pairs, triples and bombs the hand holds, plus the rocket when nothing else follows; a follow: pass, the bombs --
after a bomb the higher bombs --, plus the rocket when nothing else follows) and, where the hand's rank masks say more may be
legal, goes on with a tail from the planner.  Built with tests/constructed_states.py (imported, not edited); numpy only, the
oracle module and its action table are handed in.  Imported by tests/test_rollout_list_cases_cpu.py (the pin: every case
has the shape it is meant to have, every forced draw was found) and tests/test_gpu_rollout_list_cases.py.

One CASE = (name, the actor's hand, the combination to beat or None for a lead, n0 = rows of the closed-form round,
tail = what the kernel's scalar test answers, more = whether the list really holds rows beyond the round).  tail and not
more is the superset case: the test lets the planner look and the planner finds nothing.
One TABLE per (case, wanted list index): the meta row's episode is searched (force_episode) so that the engine RNG draws
that index, every index for lists of at most 40 rows, else 0, n0 - 1, n0, n0 + 1 and n - 1."""
import numpy as np

import constructed_states as cs

R3, R4, R5, R6, R7, R8, R9, R10, RJ, RQ, RK, RA, R2, BJ, CJ = range(15)
M12, M13, M15, JOKERS = 0x0FFF, 0x1FFF, 0x7FFF, 0x6000
QUADRIC, THREE_ONE, THREE_TWO, SINGLE_LINE, DOUBLE_LINE, TRIPLE_LINE, THREE_ONE_LINE, THREE_TWO_LINE, BIGBANG, FOUR_ONE, FOUR_TWO = range(4, 15)
ID_BIGBANG = 11498
ROCKET = {BJ: 1, CJ: 1}

LEADS = [
    # name, hand, n0, tail, more
    ("lead singles", {R3: 1, R5: 1, R7: 1, R9: 1, RQ: 1, R2: 1}, 6, False, False),
    ("lead singles+pairs", {R3: 2, R5: 1, R7: 2, R10: 1, R2: 2}, 8, False, False),
    ("lead singles+pairs+rocket", {R3: 2, R5: 1, R7: 2, R10: 1, R2: 2, **ROCKET}, 11, False, False),
    ("lead one triple", {R4: 3, R8: 1, RJ: 2}, 6, True, True),
    ("lead one bomb", {R6: 4, R9: 1, RQ: 1}, 6, True, True),
    ("lead 5-run", {R5: 1, R6: 1, R7: 1, R8: 1, R9: 1, RK: 2}, 7, True, True),
    ("lead pair 3-run", {R7: 2, R8: 2, R9: 2, R2: 1}, 7, True, True),
    ("lead triple+5-run+rocket", {R3: 3, R5: 1, R6: 1, R7: 1, R8: 1, R9: 1, **ROCKET}, 10, True, True),
    ("lead 20 cards planes+quad", {R3: 1, R4: 1, R5: 2, R6: 3, R7: 3, R9: 1, RJ: 4, RQ: 2, RK: 1, RA: 1, R2: 1}, 20, True, True),
    ("lead one card", {R8: 1}, 1, False, False),
    ("lead one pair", {R8: 2}, 2, False, False),
    ("lead two singles", {R8: 1, RQ: 1}, 2, False, False),
    ("lead the rocket", dict(ROCKET), 3, False, False),
    ("lead a triple alone", {R8: 3}, 3, True, False),    # 3+1 and 3+2 have no kicker: the planner looks and finds nothing
]

# the combination to beat per category (low values: the deck still holds higher ones)
BEATS = {
    "bomb": {R5: 4},
    "rocket": dict(ROCKET),
    "3+1": {R5: 3, R10: 1},
    "3+2": {R5: 3, R10: 2},
    "single chain": {R4: 1, R5: 1, R6: 1, R7: 1, R8: 1},
    "double chain": {R4: 2, R5: 2, R6: 2},
    "triple chain": {R5: 3, R6: 3},
    "plane 3+1": {R5: 3, R6: 3, R10: 1, RJ: 1},
    "plane 3+2": {R5: 3, R6: 3, R10: 2, RJ: 2},
    "four+1": {R5: 4, R10: 1, RJ: 1},
    "four+2": {R5: 4, R10: 2, RJ: 2},
}
PASS = {R9: 1, RQ: 2, R2: 1}
BOMB = {R9: 1, RQ: 2, RK: 4}
BOMBS_ROCKET = {R9: 1, RK: 4, RA: 4, **ROCKET}
LOWBOMB = {R9: 1, RQ: 2, R3: 4}              # (a bomb is a triple too: behind a triple-based combination only a LOWER
LOWBOMBS_ROCKET = {R9: 1, R3: 4, R4: 4, **ROCKET}    #  bomb leaves the list without a tail)
BR = {RK: 4, **ROCKET}     # what every "higher combination" hand holds besides: a bomb and the rocket
FOLLOWS = [
    # category, tag, hand, n0, tail, more
    ("bomb", "pass", PASS, 1, False, False),
    ("bomb", "higher bomb", BOMB, 2, False, False),
    ("bomb", "higher bombs+rocket", BOMBS_ROCKET, 4, False, False),
    ("bomb", "lower bomb", {R3: 4, R9: 1}, 1, False, False),
    ("bomb", "lower and higher bomb+rocket", {R3: 4, R9: 4, **ROCKET}, 3, False, False),
    ("rocket", "pass", PASS, 1, False, False),
    ("rocket", "bomb", BOMB, 1, False, False),
    ("rocket", "two bombs+triple", {R9: 3, RK: 4, RA: 4}, 1, False, False),
    ("3+1", "pass", PASS, 1, False, False),
    ("3+1", "bomb below", LOWBOMB, 2, False, False),
    ("3+1", "bombs below+rocket", LOWBOMBS_ROCKET, 4, False, False),
    ("3+1", "higher", {R8: 3, R9: 1, **BR}, 2, True, True),
    ("3+1", "triple without kicker", {R8: 3}, 1, True, False),
    ("3+1", "lower triple", {R3: 3, R9: 1}, 1, False, False),
    ("3+2", "pass", PASS, 1, False, False),
    ("3+2", "bomb below", LOWBOMB, 2, False, False),
    ("3+2", "bombs below+rocket", LOWBOMBS_ROCKET, 4, False, False),
    ("3+2", "higher", {R8: 3, R9: 2, **BR}, 2, True, True),
    ("3+2", "triple without pair", {R8: 3, R9: 1}, 1, True, False),
    ("single chain", "pass", PASS, 1, False, False),
    ("single chain", "bomb", BOMB, 2, False, False),
    ("single chain", "bombs+rocket", BOMBS_ROCKET, 4, False, False),
    ("single chain", "higher", {R6: 1, R7: 1, R8: 1, R9: 1, R10: 1, **BR}, 2, True, True),
    ("single chain", "run not higher", {R3: 1, R4: 1, R5: 1, R6: 1, R7: 1, R9: 1}, 1, False, False),
    ("single chain", "higher run too short", {R8: 1, R9: 1, R10: 1, RJ: 1, RK: 1}, 1, False, False),
    ("double chain", "pass", PASS, 1, False, False),
    ("double chain", "bomb", BOMB, 2, False, False),
    ("double chain", "bombs+rocket", BOMBS_ROCKET, 4, False, False),
    ("double chain", "higher", {R7: 2, R8: 2, R9: 2, **BR}, 2, True, True),
    ("double chain", "run not higher", {R3: 2, R4: 2, R5: 2, RQ: 1}, 1, False, False),
    ("triple chain", "pass", PASS, 1, False, False),
    ("triple chain", "bomb below", LOWBOMB, 2, False, False),
    ("triple chain", "bombs below+rocket", LOWBOMBS_ROCKET, 4, False, False),
    ("triple chain", "higher", {R7: 3, R8: 3, **BR}, 2, True, True),
    ("triple chain", "run not higher", {R3: 3, R4: 3, RQ: 1}, 1, False, False),
    ("plane 3+1", "pass", PASS, 1, False, False),
    ("plane 3+1", "bomb below", LOWBOMB, 2, False, False),
    ("plane 3+1", "bombs below+rocket", LOWBOMBS_ROCKET, 4, False, False),
    ("plane 3+1", "higher", {R7: 3, R8: 3, R9: 1, RJ: 1, **BR}, 2, True, True),
    ("plane 3+1", "triples without kickers", {R7: 3, R8: 3}, 1, True, False),
    ("plane 3+2", "pass", PASS, 1, False, False),
    ("plane 3+2", "bomb below", LOWBOMB, 2, False, False),
    ("plane 3+2", "bombs below+rocket", LOWBOMBS_ROCKET, 4, False, False),
    ("plane 3+2", "higher", {R7: 3, R8: 3, R9: 2, RJ: 2, **BR}, 2, True, True),
    ("plane 3+2", "triples without pairs", {R7: 3, R8: 3, R9: 1, RJ: 1}, 1, True, False),
    ("four+1", "pass", PASS, 1, False, False),
    ("four+1", "bomb below", LOWBOMB, 2, False, False),
    ("four+1", "bombs below+rocket", LOWBOMBS_ROCKET, 4, False, False),
    ("four+1", "higher", {R8: 4, R9: 1, RJ: 1, **ROCKET}, 2, True, True),
    ("four+1", "quad without kickers", {R8: 4}, 2, True, False),
    ("four+2", "pass", PASS, 1, False, False),
    ("four+2", "bomb below", LOWBOMB, 2, False, False),
    ("four+2", "bombs below+rocket", LOWBOMBS_ROCKET, 4, False, False),
    ("four+2", "higher", {R8: 4, R9: 2, RJ: 2, **ROCKET}, 2, True, True),
    ("four+2", "quad without pairs", {R8: 4, R9: 1, RJ: 1}, 2, True, False),
]


def _counts(d):
    c = np.zeros(15, np.int64)
    for r, k in d.items():
        c[r] = k
    return c


def _mask(counts, k):
    return int(sum(1 << r for r in range(15) if counts[r] >= k))


def _run_starts(m, length):
    x = m
    for i in range(1, length):
        x &= m >> i
    return x


def scalar_split(hand, cat, value, length):
    """The decision k_rollout takes on the rank masks of `hand` against the combination to beat (cat 0 = a lead), stated
    in numpy: (rows of the closed-form round, whether the planner is asked for a tail)."""
    m1, m2, m3, m4 = _mask(hand, 1) & M15, _mask(hand, 2) & M13, _mask(hand, 3) & M13, _mask(hand, 4) & M13
    pc = lambda m: bin(m).count("1")
    jokers = (m1 & JOKERS) == JOKERS
    if cat == 0:
        tail = m3 != 0 or _run_starts(m1 & M12, 5) != 0 or _run_starts(m2 & M12, 3) != 0
        return pc(m1) + pc(m2) + pc(m3) + pc(m4) + (1 if jokers and not tail else 0), tail
    above = 0 if value >= 14 else M15 & ~((2 << value) - 1)
    if cat == QUADRIC:
        return 1 + pc(m4 & above) + (1 if jokers else 0), False
    if cat == BIGBANG:
        return 1, False
    may = 0
    if cat in (THREE_ONE, THREE_TWO):
        may = m3 & above
    elif cat == SINGLE_LINE:
        may = _run_starts(m1 & M12, length) & above
    elif cat == DOUBLE_LINE:
        may = _run_starts(m2 & M12, length) & above
    elif cat in (TRIPLE_LINE, THREE_ONE_LINE, THREE_TWO_LINE):
        may = _run_starts(m3 & M12, length) & above
    elif cat in (FOUR_ONE, FOUR_TWO):
        may = m4 & above
    tail = may != 0
    return 1 + pc(m4) + (1 if jokers and not tail else 0), tail


class Cases:
    """name / hand [C,15] / beat id [C] (0 = a lead) / n0 / tail / more as declared; states [C,11,16] with episode 0;
    off / rows / ids = the oracle's lists of those states; n = list sizes"""


def build(oracle, table, both_jokers_only=False):
    """the cases of the CURRENT rule set of `oracle` (the caller holds oracle.variant(jk=...) open around this and around
    the lists' use); both_jokers_only: the cases whose actor holds both jokers"""
    rows = [(n, _counts(h), None, n0, t, m) for n, h, n0, t, m in LEADS]
    rows += [(f"follow {c}: {tag}", _counts(h), _counts(BEATS[c]), n0, t, m) for c, tag, h, n0, t, m in FOLLOWS]
    if both_jokers_only:
        rows = [r for r in rows if r[1][BJ] and r[1][CJ]]
    C = len(rows)
    out = Cases()
    out.name = [r[0] for r in rows]
    out.hand = np.stack([r[1] for r in rows])
    beat = np.stack([np.zeros(15, np.int64) if r[2] is None else r[2] for r in rows])
    out.beat = np.maximum(table.lookup(beat), 0)
    assert np.array_equal(table.rows[out.beat], beat), "a combination to beat is no action"
    out.n0 = np.array([r[3] for r in rows])
    out.tail = np.array([r[4] for r in rows])
    out.more = np.array([r[5] for r in rows])
    lead = out.beat == 0
    # a lead: the lord (role 1) at ply 3, every recent row empty; a follow: down (role 2) at ply 4 behind the lord's handout
    role = np.where(lead, 1, 2)
    rng = np.random.default_rng(5)
    avail = cs.DECK - out.hand - beat
    assert np.all(avail >= 0), "hand + combination to beat exceed the deck"
    hands = np.zeros((C, 3, 15), np.int64)
    hist = np.zeros((C, 3, 15), np.int64)
    hands[np.arange(C), role] = out.hand
    for k in range(2):                              # the two other players hold a third of the rest each (at most 10 cards)
        o = (role + 1 + k) % 3
        got = cs.draw_cards(rng, avail, np.minimum(avail.sum(1) // 3, 10))
        hands[np.arange(C), o] = got
        avail = avail - got
    assert np.all(hands.sum(2) > 0)
    hist[:, 1] = beat                               # the lord has played the combination to beat ...
    hist[np.arange(C), np.where(lead, 0, 1)] += avail   # ... and the rest of the deck lies in one history
    s = cs.pack_state(hands, hist, role=role, ply=np.where(lead, 3, 4))
    s[~lead, cs.F_RECENT0 + 1] = table.row16[out.beat[~lead]]
    cs.check_consistent(s, table)
    out.states = s
    out.off, out.rows, out.ids = cs.oracle_lists(oracle, s)
    out.n = np.diff(out.off).astype(np.int64)
    return out


def wanted(n, n0):
    """the list indices to play of a list of n rows whose closed-form round has n0"""
    if n <= 40:
        return list(range(n))
    return sorted({0, n0 - 1, n0, n0 + 1, n - 1})


def tables(cases, total=None):
    """One table per (case, wanted index), in case order; with `total`, that sequence repeated until there are `total`
    tables.  Table t has global id GID_BASE + t, so every copy of a case needs (and gets) an episode of its own.
    Returns (states, case number [T], wanted index [T], trials [T]: -1 where force_episode found no episode)."""
    case, index = [], []
    for c in range(len(cases.n)):
        for j in wanted(int(cases.n[c]), int(cases.n0[c])):
            case.append(c)
            index.append(j)
    case, index = np.array(case), np.array(index)
    if total is not None:
        reps = -(-total // len(case))
        case, index = np.tile(case, reps)[:total], np.tile(index, reps)[:total]
    states, trials = cs.force_episode(cases.states[case], index, cases.n[case], cs.SEED, cs.GID_BASE)
    return states, case, index, trials
