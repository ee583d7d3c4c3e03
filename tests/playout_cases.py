"""Constructed roots for k_playout / k_playout_choose (csrc/ddz_playout.h) and the conditions that say what the playouts
from them walk through.  numpy only: built with tests/constructed_states.py (imported, not edited), the oracle module and its
action table are handed in; the CURRENT rule set of `oracle` is used (the caller holds oracle.variant(jk=...) open around
build() and reference()).  Imported by tests/test_playout_cases_cpu.py (shape, consistency, coverage) and
tests/test_gpu_playout_cases.py (the kernels against tests/playout_reference.py on these roots).  Every rng stream is fixed:
the same states in every process.

A SET is one batch of tables that is run as one env: name, states uint8 [T,11,16], names [T], kind [T], K, seed, gid_base.
  roots    every (category, length) a follower can face, as the combination to beat at the root:
             per group, per role L that can lead it (any role up to 16 cards, the lord alone 18; a 20-card combination ends the
             game, nobody ever faces one), an actor's hand WITH an answer in kind (where the deck holds one next to the
             combination) and one WITHOUT, so that pass, bombs and the rocket are the whole list; each as follow1 (the actor is
             L + 1: step) and as follow2 (the actor is L + 2 and L + 1 has passed: step, then skip_turn).  What else the hand
             holds depends on L -- up: a bomb and the rocket, the lord: a bomb, down: the rocket -- so the rocket is met with a
             planner's tail in front of it and without one.
           "lead *": the state before the step of one answer form per group (the leader holds the combination and a card or two:
             the follower's answer in kind is then picked, or not, at a NON-root ply), one lead_exact state per category, and
             the rocket on a lead without a tail (lane 54 of the closed-form round).
  ply      some of `roots` with the u16 ply counter about to wrap: at the first drawn ply, the second, the fourth
  deals    fresh deals (and one or two random plies on): the wrap inside the first block of 64 draws, on the last lane of it,
           on the first and on the second lane of the second block (a playout of 66 moves or more refills twice)
  long     the lead root with the longest list (LONG_MIN or more: the `k << 9 | j` packing has j >= 256), K = 2
  outside  OUTSIDE the domain, by name: a running table whose actor's hand is empty, as a lead and facing a single
  jk sets  (joker-kicker rule set) roots again, "jk leads" = lead roots that hold a quad or two adjacent triples with both
           jokers -- and roots whose SECOND player holds them --, and a batch of 8 fresh deals"""
import numpy as np

import constructed_states as cs
import playout_reference as pr

EMPTY, SINGLE, DOUBLE, TRIPLE, QUADRIC, THREE_ONE, THREE_TWO, SINGLE_LINE, DOUBLE_LINE, TRIPLE_LINE, THREE_ONE_LINE, \
    THREE_TWO_LINE, BIGBANG, FOUR_ONE, FOUR_TWO = range(15)
CATEGORIES = tuple(range(1, 15))
BJ, CJ = 13, 14
NA_PLAIN = 13527                 # ids from here on are the joker-kicker rows
LONG_MIN = 257
OUTSIDE = ("outside: empty hand leads", "outside: empty hand faces a single")
SEED, GID_BASE = 13, 2 ** 32 + 77
PLIES8 = (0, 1, 2, 5, 11, 23, 40, 60)
JK_DEAL_SEED = 21                # (a deal whose eighth table is still running after 60 random plies)
# root plies of the `ply` set: the wrap falls at the first (0xFFFF), the second (0xFFFE) and the fourth (0xFFFC) drawn ply
PLY_SMALL = (0xFFFF, 0xFFFE, 0xFFFC)
# fresh deals: (name, seed of the deal, random plies on, root ply).  Lane l of a block of 64 draws holds the draw of ply
# ply0 + 1 + l (first block) or ply0 + 65 + l (second): the wrap sits on lane 30, on lane 63, on lane 0 and on lane 1 of the
# second block.  The lord moves at plies 0 mod 3, down 1 mod 3, up 2 mod 3 (game.py:173-181): the pairing is kept.
DEALS = (("deal: wrap inside the first block", 31, 0, 0xFFE1), ("deal: wrap on the last lane of the first block", 32, 0, 0xFFC0),
         ("deal: wrap at the second refill", 33, 2, 0xFFBF), ("deal: wrap behind the second refill", 50, 1, 0xFFBE))


class Set:
    def __init__(self, name, states, names, kind, K, group=None):
        self.name, self.states, self.names, self.kind, self.K = name, np.ascontiguousarray(states), list(names), list(kind), K
        self.group = list(group) if group is not None else [None] * len(self.names)
        self.seed, self.gid_base = SEED, GID_BASE
        self.T = len(self.states)
        assert self.T == len(self.names) == len(self.kind) == len(self.group) and len(set(self.names)) == self.T, name


def reference(oracle, s):
    """(wins, totals, Trace) of a set"""
    return pr.playouts(oracle, s.states, s.K, seed=s.seed, gid_base=s.gid_base, trace=True)


def groups(table):
    """the (category, length) groups a follower can face: everything but the 20-card combinations"""
    g = sorted(set(zip(table.cat[1:].tolist(), table.length[1:].tolist())))
    return [x for x in g if table.cards[(table.cat == x[0]) & (table.length == x[1])].min() < cs.DEALT[1]]


def _counts(d):
    c = np.zeros(15, np.int64)
    for r, k in d.items():
        c[r] = k
    return c


def in_kind(table, members, beat, hand):
    """does `hand` hold a member of the group that beats `beat` in kind (same category and length, higher value)"""
    m = members[table.value[members] > table.value[beat]]
    return bool(np.all(table.rows[m] <= hand, axis=1).any())


def mid_game(table, rng, hands, role, i):
    """one consistent running table in which `role` leads mid-game: hands {role: counts}, every recent row empty, the rest of
    the deck split over the histories by what each role has played (as constructed_states.lead_exact does)"""
    h = np.stack([hands[r] for r in range(3)])[None]
    assert np.all(h.sum(2) > 0) and np.all(h.sum(2) <= np.array(cs.DEALT))
    avail = cs.DECK - h[0].sum(0)
    assert np.all(avail >= 0)
    hist = np.zeros((1, 3, 15), np.int64)
    for o in (0, 1):
        hist[0, o] = cs.draw_cards(rng, avail[None], cs.DEALT[o] - h[0, o].sum())[0]
        avail = avail - hist[0, o]
    hist[0, 2] = avail
    assert avail.sum() == cs.DEALT[2] - h[0, 2].sum()
    return cs.pack_state(h, hist, role=role, ply=3 + (role + 2) % 3 + 3 * (i % 5))


def _draw(rng, avail, k):
    return cs.draw_cards(rng, avail[None], min(int(k), int(avail.sum())))[0]


def _pieces(rng, avail, bomb, rocket):
    """a bomb of a random rank and / or the rocket out of `avail`, or None where it holds none"""
    p = np.zeros(15, np.int64)
    if bomb:
        r = np.flatnonzero(avail[:13] >= 4)
        if len(r) == 0:
            return None
        p[rng.choice(r)] = 4
    if rocket:
        if avail[BJ] < 1 or avail[CJ] < 1:
            return None
        p[BJ] = p[CJ] = 1
    return p


def _designed(table, rng, members, answer, bomb, rocket):
    """(beat id, the actor's hand) for a group: with an answer in kind or without one, with the pieces asked for where the
    deck and the form allow them (dropped one by one where 300 draws found none); None: the group has no such form"""
    for bomb, rocket in ((bomb, rocket), (bomb, False), (False, rocket), (False, False)):
        for _ in range(300):
            beat = int(rng.choice(members))
            avail = cs.DECK - table.rows[beat]
            hand = np.zeros(15, np.int64)
            if answer:
                m = members[(table.value[members] > table.value[beat]) & np.all(table.rows[members] <= avail, axis=1)
                            & (table.cards[members] < cs.DEALT[0])]
                if len(m) == 0:
                    continue
                hand = table.rows[int(rng.choice(m))].copy()
            p = _pieces(rng, avail - hand, bomb, rocket)
            if p is None:
                continue
            hand = hand + p
            hand = hand + _draw(rng, avail - hand, rng.integers(1, 4))
            if hand.sum() > cs.DEALT[0] or hand.sum() == 0 or in_kind(table, members, beat, hand) != answer:
                continue
            return beat, hand
    return None


def follow_roots(table, rng):
    """the roots of (a): lists of (name, kind, group, state)"""
    out = []
    for gi, g in enumerate(groups(table)):
        members = np.flatnonzero((table.cat == g[0]) & (table.length == g[1]))
        cards = int(table.cards[members[0]])
        for L in range(3):
            if cards >= cs.DEALT[L]:
                continue
            for answer in (True, False):
                d = _designed(table, rng, members, answer, bomb=L in (0, 1), rocket=L in (0, 2))
                if d is None:
                    assert answer, g        # a form without an answer in kind exists for every group
                    continue
                beat, hand = d
                avail = cs.DECK - table.rows[beat] - hand
                lead = table.rows[beat] + _draw(rng, avail, min(rng.integers(1, 3), cs.DEALT[L] - cards))
                other = _draw(rng, avail - (lead - table.rows[beat]), rng.integers(1, 4))
                tag = "%s len %d led by %d, %s" % (g[0], g[1], L, "answer" if answer else "none")
                for passes in (0, 1):
                    a, o = (L + 1 + passes) % 3, (L + 2 - passes) % 3
                    base = mid_game(table, rng, {L: lead, a: hand, o: other}, L, gi)
                    s = cs.step(base, table, [beat])
                    if passes:
                        s = cs.skip_turn(s)
                    assert cs.running(s).all()
                    out.append(("follow%d %s" % (passes + 1, tag), "follow%d" % (passes + 1), g, s[0]))
                    if answer and passes == 0 and L == (gi % 3 if cards < cs.DEALT[0] else 1):
                        out.append(("lead before " + tag, "lead", None, base[0]))
    return out


def lead_roots(table, rng):
    """one lead_exact state per category (the actor holds exactly a combination of it: the lowest id of the category's
    longest group the role can hold) and the rocket on leads without a tail"""
    out = []
    for c in CATEGORIES:
        ids = np.flatnonzero((table.cat == c) & (table.cards < cs.DEALT[c % 3]))
        a = ids[table.length[ids] == table.length[ids].max()][:1]
        _, s = cs.lead_exact(table, c % 3, rng, a)
        out.append(("lead exact category %d" % c, "lead", None, s[0]))
    for i, (role, h) in enumerate(((1, {3: 2, 5: 1, 8: 2, 11: 1, BJ: 1, CJ: 1}), (0, {BJ: 1, CJ: 1}), (2, {6: 1, BJ: 1, CJ: 1}))):
        hand = _counts(h)
        avail = cs.DECK - hand
        a = _draw(rng, avail, 3)
        b = _draw(rng, avail - a, 4)
        s = mid_game(table, rng, {role: hand, (role + 1) % 3: a, (role + 2) % 3: b}, role, i)
        out.append(("lead rocket without a tail %d" % i, "lead rocket", None, s[0]))
    return out


def jk_roots(table, rng):
    """lead roots whose actor, or whose second player, holds a quad or two adjacent triples together with both jokers"""
    out = []
    for i in range(9):
        role, r = i % 3, 2 + i
        quad = i % 2 == 0
        rich = _counts({r: 4, BJ: 1, CJ: 1} if quad else {r: 3, r + 1: 3, BJ: 1, CJ: 1})
        # the other form's root actor leads a lower combination of the same kind with plain kickers: the second player's
        # list is then pass, the bomb, the joker-kicker row and the rocket
        low = _counts({0: 4, 11: 1, 12: 1} if quad else {0: 3, 1: 3, 11: 1, 12: 1})
        for second in (False, True):
            first = (low + _draw(rng, cs.DECK - low - rich, 1)) if second else rich + _draw(rng, cs.DECK - rich, 1)
            nxt = rich if second else _draw(rng, cs.DECK - first, 3)
            third = _draw(rng, cs.DECK - first - nxt, 3)
            s = mid_game(table, rng, {role: first, (role + 1) % 3: nxt, (role + 2) % 3: third}, role, i)
            out.append(("jk lead %d %s %s" % (i, "quad" if quad else "triples", "second" if second else "actor"), "lead", None, s[0]))
    return out


def deal_states(oracle, seed, gid_base, plies):
    """len(plies) tables from reset(), table i advanced by plies[i] plies of the engine's random policy; all still running"""
    ref = oracle.OracleEnv(len(plies), seed=seed, gid_base=gid_base)
    ref.reset()
    for it in range(max(plies)):
        ref.legal()
        ref.step(oracle.STEP_IDS, np.where(np.array(plies) > it, -1, -2).astype(np.int32), auto_reset=False)   # -2: no move
    st = ref.state.reshape(len(plies), 11, 16).copy()
    assert cs.running(st).all() and cs.meta_ply(st).tolist() == list(plies)
    return st


def _set(name, rows, K):
    return Set(name, np.stack([r[3] for r in rows]), [r[0] for r in rows], [r[1] for r in rows], K, [r[2] for r in rows])


def ply_set(roots):
    """three roots of `roots` per ply of PLY_SMALL, whose actor is the role that moves at that ply: the follow1 and follow2
    forms that hold an answer in kind, longest hands first (the playouts must reach the wrap)"""
    role = roots.states[:, cs.F_META, cs.M_ROLE]
    cards = roots.states[:, 0:3, 15].astype(np.int64).sum(1)
    rows = []
    for p in PLY_SMALL:
        ok = [t for t in np.argsort(-cards, kind="stable") if (role[t] + 2) % 3 == p % 3 and roots.kind[t].startswith("follow")
              and roots.names[t].endswith("answer")]
        for t in ok[:2] + [x for x in ok[2:] if roots.kind[x] != roots.kind[ok[0]]][:1]:
            s = roots.states[t:t + 1].copy()
            cs.set_ply(s, [p])
            rows.append(("ply %#x: %s" % (p, roots.names[t]), roots.kind[t], roots.group[t], s[0]))
    return _set("ply", rows, 2)


def outside_set(table):
    """the two tables outside the domain: running, the actor's hand empty"""
    rng = np.random.default_rng(44)
    rows = []
    for name, role in zip(OUTSIDE, (1, 2)):
        hands = {role: _counts({7: 1}), (role + 1) % 3: _counts({2: 2, 9: 1}), (role + 2) % 3: _counts({4: 1, 12: 1})}
        s = mid_game(table, rng, hands, role, 0)
        s[0, cs.F_HAND0 + role] = 0                   # the actor's last card goes to its history: the hand is empty, done stays 0
        s[0, cs.F_HIST0 + role, 7] += 1
        s[0, cs.F_TAKEN, 7] += 1
        if role == 2:                                 # ... facing the single the lord played last
            r = int(np.flatnonzero(s[0, cs.F_HIST0 + 1, :15])[0])
            s[0, cs.F_RECENT0 + 1, r], s[0, cs.F_RECENT0 + 1, 15] = 1, SINGLE
        rows.append((name, "outside", None, s[0]))
    return _set("outside", rows, 2)


def long_root(oracle, table):
    """the state of families()['lead0'] with the longest list (the same rng stream; force_episode writes the episode alone,
    which no playout reads, and oracle.beats only confirms the planted answers)"""
    ids = np.arange(1, table.n)
    s0, _ = cs.lead0(table, ids, np.random.default_rng(0))
    n, _, _ = pr.root_lists(oracle, s0)
    t = int(np.argmax(n))
    return Set("long", s0[t:t + 1], ["long: lead0 of id %d, %d moves" % (ids[t], n[t])], ["lead"], 2)


def build(oracle, table, jk=False):
    """{name: Set} of the current rule set"""
    roots = _set("roots", follow_roots(table, np.random.default_rng(41)) + lead_roots(table, np.random.default_rng(42)), 2)
    if jk:
        return {"roots": roots, "jk leads": _set("jk leads", jk_roots(table, np.random.default_rng(43)), 2),
                "jk deals": Set("jk deals", deal_states(oracle, JK_DEAL_SEED, GID_BASE, PLIES8), ["jk deal +%d" % p for p in PLIES8],
                                ["deal"] * len(PLIES8), 1)}
    deals = []
    for name, seed, on, ply in DEALS:
        s = deal_states(oracle, seed, 0, (on,))
        cs.set_ply(s, [ply])
        deals.append((name, "deal", None, s[0]))
    return {"roots": roots, "ply": ply_set(roots), "deals": _set("deals", deals, 2), "long": long_root(oracle, table),
            "outside": outside_set(table)}


def mapping_batch(sets, T):
    """T roots of `roots` for the mapping test: spread over the set, so follows, leads and every role are among them"""
    r = sets["roots"]
    pick = (np.arange(T) * 37 + 5) % r.T
    return Set("mapping %d" % T, r.states[pick], [r.names[t] for t in pick], [r.kind[t] for t in pick], 4)


# ---- what the playouts walk through (read from the reference's trace alone) --------------------------------------------------
def coverage(table, sets, traces):
    """{condition: witness} over the sets: witness = the name of the first case that reaches the condition, None where no
    case does.  `traces` {set name: (wins, totals, Trace)}.  An answer in kind is asked for every category but the rocket's:
    nothing beats the rocket (its pick is a condition of its own)."""
    found = {}
    want = [("root passes0=%d beats %s" % (p, g), None) for p in (0, 1) for g in groups(table)]
    want += [("non-root beats category %d" % c, None) for c in CATEGORIES]
    want += [("non-root pass", None), ("non-root bomb over a non-bomb", None), ("non-root rocket", None)]
    want += [("non-root answer in kind category %d" % c, None) for c in CATEGORIES if c != BIGBANG]
    want += [("lead picks category %d" % c, None) for c in CATEGORIES]
    want += [("lead after two passes", None), ("rocket from lane 54 at a root", None), ("66 moves or more", None),
             ("wrap at a refill", None)]
    for name, s in sets.items():
        if name == "outside":
            continue
        tr = traces[name][2]
        st = tr.steps
        case = np.array(s.names, object)[tr.t[st["copy"]]]
        root = st["s"] == 0
        beat, pick = st["beat"], st["id"]
        bc, pc = table.cat[beat], table.cat[pick]

        def hit(key, mask):
            if key not in found and mask.any():
                found[key] = case[np.flatnonzero(mask)[0]]

        passes0 = np.array([k == "follow2" for k in s.kind])[tr.t[st["copy"]]]
        for g in groups(table):
            m = root & (bc == g[0]) & (table.length[beat] == g[1])
            hit("root passes0=0 beats %s" % (g,), m & ~passes0)
            hit("root passes0=1 beats %s" % (g,), m & passes0)
        for c in CATEGORIES:
            hit("non-root beats category %d" % c, ~root & (bc == c))
            hit("lead picks category %d" % c, (beat == 0) & (pc == c))
            if c != BIGBANG:
                hit("non-root answer in kind category %d" % c, ~root & (bc == c) & (pc == c))
        hit("non-root pass", ~root & (beat > 0) & (pick == 0))
        hit("non-root bomb over a non-bomb", ~root & (beat > 0) & (bc != QUADRIC) & (pc == QUADRIC))
        hit("non-root rocket", ~root & (beat > 0) & (pc == BIGBANG))
        hit("lead after two passes", st["two_passes"])
        lane54 = np.array([k == "lead rocket" for k in s.kind])[tr.t[st["copy"]]]
        hit("rocket from lane 54 at a root", root & lane54 & (pc == BIGBANG) & (st["index"] == st["A"] - 1))
        hit("66 moves or more", tr.moves[st["copy"]] >= 66)
        hit("wrap at a refill", (st["s"] == 65) & ((st["ply"] == 0) | (st["ply"] == 0xFFFF)))
    return {k: found.get(k) for k, _ in want}


def jk_coverage(table, sets, traces):
    """{condition: witness}: a joker-kicker row (id >= NA_PLAIN) picked at a root and at a non-root ply"""
    out = {"jk id at a root": None, "jk id at a non-root ply": None}
    for name, s in sets.items():
        tr = traces[name][2]
        st = tr.steps
        for key, m in (("jk id at a root", (st["s"] == 0) & (st["id"] >= NA_PLAIN)),
                       ("jk id at a non-root ply", (st["s"] > 0) & (st["id"] >= NA_PLAIN))):
            if out[key] is None and m.any():
                out[key] = s.names[tr.t[st["copy"][np.flatnonzero(m)[0]]]]
    return out


# ---- ddz_playout_choose on constructed buffers ---------------------------------------------------------------------------------
COUNTS = (0, -5, 1, 63, 64, 65, 128, 129, 497, 512, 100000)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def choose_patterns(stride):
    """[(name, fill(c) -> wins row int32 [stride + 1] for a list of c = min(count, stride) > 0 live entries -- entry `stride`
    is what lies just beyond a full row --, first(c) -> the index of the first maximum of row[:c], stated in closed form)]"""
    j = np.arange(stride + 1)

    def two(a, b):
        def fill(c):
            w = np.full(stride + 1, 7, np.int64)
            w[[a, b]] = 9
            return w
        return fill, lambda c: a if c > a else 0

    def last_max(c):
        w = (j % 11).astype(np.int64)
        w[c - 1] = I32_MAX
        return w

    def beyond(c):
        w = (j % 5).astype(np.int64)
        w[c] = 100
        return w

    pats = [("all equal", lambda c: np.full(stride + 1, 3, np.int64), lambda c: 0),
            ("all INT32_MIN", lambda c: np.full(stride + 1, I32_MIN, np.int64), lambda c: 0),
            ("INT32_MAX at the last live index", last_max, lambda c: c - 1),
            ("equal maxima at 10 and 70",) + two(10, 70), ("equal maxima at 5 and 69",) + two(5, 69),
            ("equal maxima at 63 and 64",) + two(63, 64),
            ("all negative", lambda c: -1000 + (j % 37).astype(np.int64), lambda c: min(c - 1, 36)),
            ("a larger value just beyond the count", beyond, lambda c: min(c - 1, 4))]
    return [(n, (lambda c, f=f: f(c).astype(np.int32)), g) for n, f, g in pats]


def choose_problems(T, stride):
    """the launches of the choose test for an env of T tables: [(pattern name, counts int32 [T], ids int32 [T, stride],
    wins int32 [T, stride], want int32 [T], first int64 [T] = the closed-form index or -1)].  Every count of COUNTS meets
    every pattern; ids[t, j] = 1000 t + j.  (Nothing of a table lies beyond a full row: the value beyond the count is planted
    where the count is below the stride.)"""
    ids = (1000 * np.arange(T)[:, None] + np.arange(stride)[None, :]).astype(np.int32)
    out = []
    for name, fill, first in choose_patterns(stride):
        for lo in range(0, len(COUNTS), T):
            counts = np.array([COUNTS[(lo + t) % len(COUNTS)] for t in range(T)], np.int32)
            wins = np.zeros(T * stride + 1, np.int32)
            live = np.clip(counts.astype(np.int64), 0, stride)
            for t in range(T):
                if live[t] > 0:
                    wins[t * stride:(t + 1) * stride] = fill(int(live[t]))[:stride]
            wins = wins[:T * stride].reshape(T, stride)
            want = np.array([ids[t, int(np.argmax(wins[t, :live[t]]))] if live[t] > 0 else -1 for t in range(T)], np.int32)
            fst = np.array([first(int(live[t])) if live[t] > 0 else -1 for t in range(T)], np.int64)
            out.append((name, counts, ids, wins, want, fst))
    return out
