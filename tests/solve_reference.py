"""Solve spec v1 restated on the CPU oracle, twice and independently: what ddz_solve / ddz_solve_choose must
give.  numpy and the oracle module (handed in: oracle.legal, the action table) only; nothing here touches the GPU library.

  exact()  plain recursive minimax of the open-hand game with an unbounded dictionary memo.  It knows nothing of budgets,
           tables, chunks or node counts: the value of every root move, a fact about the game.
  spec()   the spec word for word: per (table, world, chunk) one direct-mapped, always-replaced table of tt_entries entries
           that starts empty and is shared by the chunk's root moves in ascending order; per root move a budget of nodes;
           children in list order, the cut at the first child that wins for the mover's side, no cut among the root moves.
           -> n, wins, unknown, totals = {nodes, table hits, root moves solved, root moves unknown}, status.

  position   (hands by role, the combination to beat as its 15 counts or None, the passes since it was played, the mover);
             two passes hand the lead back: (None, 0).  Roles 0 up / 1 lord / 2 down, the turn goes role -> (role + 1) % 3.
  value      the mover whose hand empties wins for its side (the lord alone, or either farmer)
  node       a position ENTERED: the budget test, nodes += 1, the probe -- in this order.  A child whose move empties the
             mover's hand is not entered.
  key        x = hc | mover << 60, y = hn, z = hp, w = cb | passes << 60 (0 for the lead position); hc / hn / hp the hands
             of the mover, the next and the previous player and cb the combination to beat as 15 nibbles, rank r at bit 4r
  slot       h = x*K1 ^ y*K2 ^ z*K3 ^ w*K4; h ^= h >> 29; h *= K5; h ^= h >> 32 (mod 2^64); (h mod 2^32) & (tt_entries - 1)
  hidden     world k of playout spec v2 (playout_hidden_reference.worlds) replaces the opponents' rows; wins / unknown add up
spec(trace=True) also says what the searches walked through (class Trace): the tests' coverage conditions read it."""
import sys

import numpy as np

import playout_hidden_reference as phr

ROW, NFIELDS = 16, 11
F_HAND0, F_RECENT0, F_TAKEN, F_META = 0, 6, 9, 10
M_ROLE, M_DONE, M_DEALT = 0, 1, 6
STRIDE = 512
MAX_CARDS, MAX_DEPTH = 20, 60          # DDZ_SOLVE_MAX_CARDS, DDZ_SOLVE_MAX_DEPTH
STATUS_DOMAIN, STATUS_DEPTH = 64, 256
K1, K2, K3, K4, K5 = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0xBF58476D1CE4E5B9)
M64 = (1 << 64) - 1

sys.setrecursionlimit(max(sys.getrecursionlimit(), 4000))


def slot(x, y, z, w, tt_entries):
    h = ((x * K1) ^ (y * K2) ^ (z * K3) ^ (w * K4)) & M64
    h ^= h >> 29
    h = (h * K5) & M64
    h ^= h >> 32
    return (h & 0xFFFFFFFF) & (tt_entries - 1)


def nib(counts):
    return sum(int(c) << (4 * r) for r, c in enumerate(counts))


def unnib(word):
    return tuple((word >> (4 * r)) & 15 for r in range(15))


class Rules:
    """the oracle's lists, cached: moves(hand, last) -> [(action id, hand after it, its 15 counts)] in list order"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.rows, self.info = oracle.action_table()
        self.row15 = [tuple(int(x) for x in r[:15]) for r in self.rows]
        self.cache, self.cats = {}, {}

    def cat_of(self, row15):
        if row15 not in self.cats:
            self.cats[row15] = int(self.info[self.oracle.lookup(np.array(row15 + (0,), np.int8)), 0])
        return self.cats[row15]

    def moves_nib(self, hand, last):
        """the same list on nibble words: [(action id, hand after it, its cards)], last = 0 for a lead"""
        k = (hand, last)
        m = self.cache.get(k)
        if m is None:
            m = self.cache[k] = [(a, nib(left), nib(row)) for a, left, row in self.moves(unnib(hand), unnib(last) if last else None)]
        return m

    def moves(self, hand, last):
        k = (hand, last)
        m = self.cache.get(k)
        if m is None:
            ids = self.oracle.legal(np.array(hand + (0,), np.int8), None if last is None else np.array(last + (0,), np.int8))
            m = self.cache[k] = [(int(a), tuple(h - c for h, c in zip(hand, self.row15[a])), self.row15[a]) for a in ids]
        return m


_rules = {}


def rules(oracle):
    k = oracle.num_actions()
    if k not in _rules:
        _rules[k] = Rules(oracle)
    return _rules[k]


def decode(state):
    """(running, role, hands by role, the combination to beat or None, passes) as the open form reads a table"""
    s = np.asarray(state, np.uint8).reshape(NFIELDS, ROW)
    m = s[F_META]
    run = bool(m[M_DEALT]) and not m[M_DONE]
    role = int(m[M_ROLE]) if m[M_ROLE] <= 2 else 0
    hands = tuple(tuple(int(x) for x in s[F_HAND0 + r, :15]) for r in range(3))
    last, passes = None, 0
    for p, r in enumerate(((role + 2) % 3, (role + 1) % 3)):
        if s[F_RECENT0 + r, :15].any():
            last, passes = tuple(int(x) for x in s[F_RECENT0 + r, :15]), p
            break
    return run, role, hands, last, passes


def same_side(a, b):
    return (a == 1) == (b == 1)


def after(hands, last, passes, mover, move):
    """the position behind `move` = (id, hand after, counts) of the mover, or None where the move empties the hand"""
    aid, left, row = move
    if aid == 0:
        passes += 1
        if passes >= 2:
            last, passes = None, 0
    else:
        if not any(left):
            return None
        hands = hands[:mover] + (left,) + hands[mover + 1:]
        last, passes = row, 0
    return hands, last, passes, (mover + 1) % 3


# ---- (a) the exact value: plain minimax, an unbounded memo
def exact_root(oracle, state, memo=None):
    """[the ROOT ACTOR's side wins behind root move j] for one open table (list order), [] for an idle one"""
    R = rules(oracle)
    run, role, hands, last, passes = decode(state)
    if not run:
        return []
    memo = {} if memo is None else memo

    def wins(pos):        # the mover's side wins
        v = memo.get(pos)
        if v is None:
            hands, last, passes, mover = pos
            v = False
            for mv in R.moves(hands[mover], last):
                nxt = after(hands, last, passes, mover, mv)
                if nxt is None or wins(nxt) == same_side(nxt[3], mover):
                    v = True
                    break
            memo[pos] = v
        return v

    out = []
    for mv in R.moves(hands[role], last):
        nxt = after(hands, last, passes, role, mv)
        out.append(True if nxt is None else wins(nxt) == same_side(nxt[3], role))
    return out


def exact(oracle, states, stride=STRIDE):
    """-> (n int32 [T], wins int32 [T, stride]) of the open form with no budget: n = the list size of every running table"""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    n, wins = np.zeros(len(states), np.int32), np.zeros((len(states), stride), np.int32)
    for t, s in enumerate(states):
        w = exact_root(oracle, s)
        n[t] = len(w)
        wins[t, :len(w)] = w
    return n, wins


# ---- (b) the spec
class Trace:
    """what the searches of one spec() call walked through: leads / follows = {category led}, {(category to beat, category
    of the answer; 0 = pass)} over every move tried, the root's included; tails = the categories of tried children that a closed-form round does
    not hold (lines, planes, anything with kickers), split by lead / follow; lead_backs = positions entered whose lead follows
    two passes; root_lead_backs = root moves that are the second pass; hits / transpositions = probes that hit / that hit an
    entry stored under another path; replaced = stores over an entry in use with another key; depth = the deepest frame;
    per (t, k, j): nodes"""

    def __init__(self):
        self.leads, self.follows, self.tail_lead, self.tail_follow = set(), set(), set(), set()
        self.lead_backs = self.root_lead_backs = self.hits = self.transpositions = self.replaced = self.depth = 0
        self.farmer_for_partner = 0
        self.nodes = {}


class _Unknown(Exception):
    pass


ROUND_CATS = (0, 1, 2, 3, 4, 12)     # what the closed-form round of a list holds: pass, groups of one rank, the rocket


def _solve_item(R, role, hands, last, passes, js, budget, tt_entries, trace, tag):
    """one (table, world, chunk): -> {j: (won, unknown, nodes)}, hits.  A position is held as the key's own words: the hands
    in turn order and the combination to beat as nibble words (0 = a lead), the passes, the mover."""
    tt = {}
    cat = R.info[:, 0]
    ctx = {"nodes": 0, "hits": 0}
    mask, K = tt_entries - 1, (K1, K2, K3, K4, K5)

    def tried(aid, cb):
        c = int(cat[aid])
        (trace.leads.add(c) if not cb else trace.follows.add((R.cat_of(unnib(cb)), c)))
        if c not in ROUND_CATS:
            (trace.tail_lead if not cb else trace.tail_follow).add(c)

    def visit(hc, hn, hp, cb, passes, mover, depth, path, passed):
        if ctx["nodes"] >= budget:
            raise _Unknown
        ctx["nodes"] += 1
        k = (hc | (mover << 60), hn, hp, cb | (passes << 60))
        h = ((k[0] * K[0]) ^ (hn * K[1]) ^ (hp * K[2]) ^ (k[3] * K[3])) & M64
        h ^= h >> 29
        h = (h * K[4]) & M64
        s = ((h ^ (h >> 32)) & 0xFFFFFFFF) & mask
        e = tt.get(s)
        if e is not None and e[0] == k:
            ctx["hits"] += 1
            if trace is not None:
                trace.hits += 1
                trace.transpositions += e[2] != path
            return e[1]
        if trace is not None:
            trace.depth = max(trace.depth, depth)
            trace.lead_backs += (not cb) and passed
        res = False
        nxt = (mover + 1) % 3
        other = (nxt == 1) != (mover == 1)       # the next mover is on the other side
        for aid, left, row in R.moves_nib(hc, cb):
            if trace is not None:
                tried(aid, cb)
            if aid == 0:
                v = visit(hn, hp, hc, 0, 0, nxt, depth + 1, path + (0,), True) if passes == 1 else \
                    visit(hn, hp, hc, cb, 1, nxt, depth + 1, path + (0,), False)
            elif left == 0:
                res = True
                if trace is not None and mover != 1 and mover != role and role != 1:
                    trace.farmer_for_partner += 1
                break
            else:
                assert depth < MAX_DEPTH
                v = visit(hn, hp, left, row, 0, nxt, depth + 1, path + (aid,) if trace is not None else path, False)
            if v != other:
                res = True
                break
        if trace is not None and e is not None:
            trace.replaced += 1
        tt[s] = (k, res, path)
        return res

    out = {}
    hc, hn, hp = nib(hands[role]), nib(hands[(role + 1) % 3]), nib(hands[(role + 2) % 3])
    cb = 0 if last is None else nib(last)
    nxt = (role + 1) % 3
    other = (nxt == 1) != (role == 1)
    moves = R.moves_nib(hc, cb)
    for j in js:
        ctx["nodes"] = 0
        aid, left, row = moves[j]
        if trace is not None:
            tried(aid, cb)
            trace.root_lead_backs += aid == 0 and passes == 1
        try:
            if aid == 0:
                won = (visit(hn, hp, hc, 0, 0, nxt, 0, (0,), True) if passes == 1 else
                       visit(hn, hp, hc, cb, passes + 1, nxt, 0, (0,), False)) != other
            else:
                won = True if left == 0 else visit(hn, hp, left, row, 0, nxt, 0, (aid,), False) != other
            out[j] = (won, False, ctx["nodes"])
        except _Unknown:
            out[j] = (False, True, ctx["nodes"])
        if trace is not None:
            trace.nodes[tag + (j,)] = ctx["nodes"]
    return out, ctx["hits"]


def spec(oracle, states, budget=65536, max_cards=12, worlds=1, hidden=False, roles=0b111, salt=0, chunks=1, tt_entries=4096,
         seed=0, gid_base=0, stride=STRIDE, trace=False):
    """ddz_solve for states uint8 [T, 11, 16] -> (n int32 [T], wins int32 [T, stride], unknown int32 [T, stride], totals
    int64 [4], status); with trace=True a Trace follows"""
    assert 1 <= budget and 1 <= max_cards <= MAX_CARDS and chunks >= 1 and tt_entries >= 1 and tt_entries & (tt_entries - 1) == 0
    assert hidden or (worlds == 1 and roles == 0b111)
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T = len(states)
    R = rules(oracle)
    n = np.zeros(T, np.int32)
    wins, unknown = np.zeros((T, stride), np.int32), np.zeros((T, stride), np.int32)
    totals, status = np.zeros(4, np.int64), 0
    tr = Trace() if trace else None
    W = phr.worlds(oracle, states, worlds, seed, gid_base, salt, roles)[0] if hidden else None
    for t, s in enumerate(states):
        run, role, hands, last, passes = decode(s)
        if not run or not (roles >> role) & 1:
            continue
        if hidden:
            _, _, unseen, n_next, n_prev, ok = phr.decode(s[None])[0]
            cards = sum(hands[role]) + n_next + n_prev
        else:
            cards = sum(sum(h) for h in hands)
        if cards > max_cards:
            n[t] = -1
            continue
        if hidden and (not ok or sum(hands[role]) < 1):
            n[t], status = -1, status | STATUS_DOMAIN
            continue
        n_root = len(R.moves(hands[role], last))
        n[t] = n_root
        for k in range(worlds):
            if hidden:
                hs = list(hands)
                hs[(role + 1) % 3] = tuple(int(x) for x in W[t, k, 0, :15])
                hs[(role + 2) % 3] = tuple(int(x) for x in W[t, k, 1, :15])
                hk = tuple(hs)
            else:
                hk = hands
            for c in range(chunks):
                js = range(c, n_root, chunks)
                if not js:
                    continue
                out, hits = _solve_item(R, role, hk, last, passes, js, budget, tt_entries, tr, (t, k))
                totals[1] += hits
                for j, (won, unk, nodes) in out.items():
                    wins[t, j] += won
                    unknown[t, j] += unk
                    totals[0] += nodes
                    totals[2] += not unk
                    totals[3] += unk
    return (n, wins, unknown, totals, status, tr) if trace else (n, wins, unknown, totals, status)


def choose(n, off, ids, wins, unknown, worlds=1):
    """ddz_solve_choose: (choice int32 [T], value int32 [T]) from the slab lists (off, ids) of the tables with n[t] > 0"""
    choice, value = np.full(len(n), -1, np.int32), np.full(len(n), -1, np.int32)
    for t in range(len(n)):
        c = int(n[t])
        if c <= 0:
            continue
        w, u = [int(x) for x in wins[t, :c]], [int(x) for x in unknown[t, :c]]
        j = min(range(c), key=lambda a: (-w[a], u[a], a))
        choice[t] = ids[off[t] + j]
        value[t] = 1 if w[j] >= worlds else 0 if not any(w) and not any(u) else -1
    return choice, value
