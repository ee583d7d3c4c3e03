"""Search spec v1 (UCT) restated on the CPU oracle: what ddz_search must count, independent of the engine.
numpy, math and the oracle module (handed in) only.

Every (table t, tree c) item owns one slot of ONE OracleEnv and a tree of Python records; the items run iteration i in
lock-step: every slot is set back to its root, then legal() -> one move per item (the selected child's list index, the
expansion index, or the playout's index from the Philox draw) -> step(STEP_CHOICE, no auto-reset), until every item has
scored.  The oracle calls are batched over the items.
  node       n = the size of its state's list, kids {list index: node}, V, W, terminal (the move into it emptied a hand)
  selection  value = W/V + c * sqrt((2 * LN[N]) / V) in np.float32, one rounding per operation, LN[N] = float32(math.log(N));
             "reference": max at the root actor's own nodes, min elsewhere; "sides": max at the root side's nodes, else the
             max of (V-W)/V + bonus; ties to the lowest list index
  expansion  the ((draw_e * u) >> 32)-th untried index, draw_e = philox((gid_lo, gid_hi, c << 16 | i, 6 << 16), key).x
  playout    index (draw * A) >> 32, draw = philox((gid_lo, gid_hi, c << 16 | i, 7 << 16 | ply), key).x, at most MAX_PLIES
             moves from the new child; unfinished scores 0
  score      1 if the winner is on the ROOT actor's side; backup V += 1, W += score on the whole path
  hidden     tree c plays on world c of playout spec v2 (playout_hidden_reference.worlds)
search(trace=True) also says what every iteration walked through: the tests' coverage conditions read it."""
import math

import numpy as np

import constructed_states as cs
import playout_hidden_reference as phr
import playout_reference as pr

ROW, NFIELDS, F_META = pr.ROW, pr.NFIELDS, pr.F_META
STRIDE = pr.STRIDE
MAX_PLIES = pr.MAX_PLIES       # DDZ_PLAYOUT_MAX_PLIES: moves applied from the new child at most
MAX_DEPTH = 192                # DDZ_SEARCH_MAX_DEPTH
MAX_BUDGET = 4096              # DDZ_SEARCH_MAX_BUDGET
LN = np.array([0.0] + [math.log(N) for N in range(1, MAX_BUDGET + 1)]).astype(np.float32)
F32 = np.float32


def value(W, V, N, c):
    """the fp32 value of a child with (V, W) under a parent with N visits: five single operations, each rounded once"""
    fv = F32(V)
    mean = F32(W) / fv
    q = (F32(2.0) * LN[N]) / fv
    return mean + F32(c) * np.sqrt(q)


class Node:
    __slots__ = ("n", "kids", "V", "W", "terminal", "winner", "depth")

    def __init__(self, depth):
        self.n, self.kids, self.V, self.W, self.terminal, self.winner, self.depth = -1, {}, 0, 0, False, -1, depth


class ProbeTable:
    """the kernel's open-addressing table (csrc/ddz_search.h), for the probe-length coverage condition only: nothing the
    search computes depends on it.  H = the power of two >= 2 * (budget + 1), slot = (key * 2654435761 mod 2^32) >> (32 -
    log2 H), linear probing; key = parent * 512 + list index + 1."""

    def __init__(self, budget):
        self.log = 1
        while (1 << self.log) < 2 * (budget + 1):
            self.log += 1
        self.slots = {}
        self.longest = 0          # the most slots any insertion stepped past

    def insert(self, parent, j):
        key = parent * 512 + j + 1
        h = ((key * 2654435761) & 0xFFFFFFFF) >> (32 - self.log)
        steps = 0
        while h in self.slots:
            h = (h + 1) & ((1 << self.log) - 1)
            steps += 1
        self.slots[h] = key
        self.longest = max(self.longest, steps)


class Item:
    def __init__(self, t, c, root, root_role, budget):
        self.t, self.c, self.root, self.root_role = t, c, root, root_role
        self.nodes = [Node(0)]
        self.probe = ProbeTable(budget)
        self.iters = []           # trace: one dict per iteration


def _own(mode, role, root_role):
    return (role == root_role) if mode == "reference" else ((role == 1) == (root_role == 1))


def select(node, nodes, mode, own, c):
    """(list index, values float32 [n], took the maximum, tied) at a fully expanded node"""
    vals = np.empty(node.n, np.float32)
    for j in range(node.n):
        k = nodes[node.kids[j]]
        w = k.W if (own or mode == "reference") else k.V - k.W
        vals[j] = value(w, k.V, node.V, c)
    take_max = own or mode == "sides"
    best = vals.max() if take_max else vals.min()
    at = np.flatnonzero(vals == best)
    return int(at[0]), vals, take_max, len(at) > 1


def search(oracle, states, budget, trees=1, mode="reference", c=0.7, seed=0, gid_base=0, salt=0, hidden=False, roles=0b111,
           stride=STRIDE, max_plies=MAX_PLIES, trace=False):
    """-> (visits int32 [T, stride], wins int32 [T, stride], totals int64 [4]) of search spec v1 for `states` uint8
    [T, 11, 16]; with trace=True -> (visits, wins, totals, items): items[k].iters[i] = {"path": node numbers from the root,
    "sel": [(depth, node, list index, took the max, tied, values)], "expand": (node, list index, n of the node) or None,
    "expand_id": the canonical id of the expansion's move (beside "expand"),
    "terminal": the path ended in a terminal node that existed before, "moves", "winner"}, items[k].nodes, .probe"""
    assert mode in ("reference", "sides") and 1 <= budget <= MAX_BUDGET and c >= 0
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T = len(states)
    visits, wins = np.zeros((T, stride), np.int32), np.zeros((T, stride), np.int32)
    totals = np.zeros(4, np.int64)
    n_root, _, _ = pr.root_lists(oracle, states, seed, gid_base)
    if hidden:
        W, part, _ = phr.worlds(oracle, states, trees, seed, gid_base, salt, roles)
        n_root = np.where(part, n_root, 0)
    items = []
    for t in np.flatnonzero(n_root > 0):
        role = int(states[t, F_META, pr.M_ROLE]) % 3
        for k in range(trees):
            root = phr.with_world(states[t], W[t, k]) if hidden else states[t].copy()
            it = Item(int(t), k, root, role, budget)
            it.nodes[0].n = int(n_root[t])
            items.append(it)
    if not items:
        return (visits, wins, totals, items) if trace else (visits, wins, totals)
    I = len(items)
    env = oracle.OracleEnv(I, seed=seed, gid_base=gid_base)
    st = env.state.reshape(I, NFIELDS, ROW)
    m = env.field(F_META)
    roots = np.stack([it.root for it in items])
    gid = np.array([int(gid_base) + it.t for it in items], np.uint64)
    tree = np.array([it.c for it in items], np.int64)
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    DESCEND, PLAYOUT, OVER = 0, 1, 2
    for i in range(budget):
        st[:] = roots
        ctr2 = (tree << 16) | i
        draw_e = cs.philox4x32_10(gid, gid >> np.uint64(32), ctr2, np.full(I, 6 << 16), *key)[0]
        phase = np.full(I, DESCEND)
        cur = [0] * I
        path = [[0] for _ in range(I)]
        made = [None] * I            # the node created by this iteration, waiting for its n
        left = np.zeros(I, np.int64)  # playout moves still allowed
        moves = np.zeros(I, np.int64)
        rec = [{"path": path[k], "sel": [], "expand": None, "terminal": False, "moves": 0, "winner": -1} for k in range(I)]
        while (phase != OVER).any():
            off, _, ids = env.legal()
            A = np.diff(off).astype(np.int64)
            ply = m[:, pr.M_PLY].astype(np.int64) | (m[:, pr.M_PLY + 1].astype(np.int64) << 8)
            done = m[:, pr.M_DONE] == 1
            sel = np.full(I, -1, np.int32)
            for k in np.flatnonzero(phase == DESCEND):
                it = items[k]
                node = it.nodes[cur[k]]
                if node.terminal:
                    assert done[k] and int(m[k, pr.M_WINNER]) == node.winner
                    rec[k]["terminal"], phase[k] = True, OVER
                    continue
                assert not done[k] and node.n == A[k]
                if node.n == 0 or node.depth == MAX_DEPTH:
                    phase[k] = OVER          # outside the domain: unfinished
                    continue
                role = int(m[k, pr.M_ROLE])
                if len(node.kids) < node.n:
                    untried = [j for j in range(node.n) if j not in node.kids]
                    j = untried[(int(draw_e[k]) * len(untried)) >> 32]
                    child = Node(node.depth + 1)
                    node.kids[j] = len(it.nodes)
                    it.probe.insert(cur[k], j)
                    rec[k]["expand"] = (cur[k], j, node.n)
                    rec[k]["expand_id"] = int(ids[off[k] + j])
                    it.nodes.append(child)
                    made[k] = child
                    child.winner = role      # (used if the move empties the hand)
                    sel[k], phase[k], left[k] = j, PLAYOUT, max_plies
                    totals[3] += 1
                else:
                    own = _own(mode, role, it.root_role)
                    j, vals, took_max, tied = select(node, it.nodes, mode, own, c)
                    rec[k]["sel"].append((node.depth, cur[k], j, took_max, tied, vals))
                    cur[k] = node.kids[j]
                    path[k].append(cur[k])
                    sel[k] = j
            # the playouts, all at once: the state behind the new child's move, then (draw * A) >> 32
            play = np.flatnonzero((phase == PLAYOUT) & (sel < 0))
            for k in play:
                if made[k] is not None:      # the first state of the playout: the child's n, or a terminal child
                    child, made[k] = made[k], None
                    if done[k]:
                        child.terminal, child.n = True, 0
                        assert int(m[k, pr.M_WINNER]) == child.winner
                    else:
                        child.n, child.winner = int(A[k]), -1
            stop = play[done[play] | (A[play] == 0) | (left[play] == 0)]
            phase[stop] = OVER
            go = play[~(done[play] | (A[play] == 0) | (left[play] == 0))]
            if len(go):
                d = cs.philox4x32_10(gid[go], gid[go] >> np.uint64(32), ctr2[go], (7 << 16) | ply[go], *key)[0]
                sel[go] = ((d * A[go].astype(np.uint64)) >> np.uint64(32)).astype(np.int32)
                left[go] -= 1
            act = np.flatnonzero(sel >= 0)
            if len(act) == 0:
                continue
            _, _, illegal, _ = env.step(pr.STEP_CHOICE, sel, auto_reset=False)
            assert not illegal[act].any()
            moves[act] += 1
        done = m[:, pr.M_DONE] == 1
        for k, it in enumerate(items):
            winner = int(m[k, pr.M_WINNER]) if done[k] else -1
            score = int(winner >= 0 and ((winner == 1) == (it.root_role == 1)))
            nodes = [it.nodes[x] for x in path[k]]
            if rec[k]["expand"] is not None:
                nodes.append(it.nodes[-1])
            for nd in nodes:
                nd.V += 1
                nd.W += score
            totals[2] += winner < 0
            rec[k]["moves"], rec[k]["winner"] = int(moves[k]), winner
            if trace:
                it.iters.append(rec[k])
        totals[0] += int(moves.sum())
        totals[1] += I
    for it in items:
        for j, x in it.nodes[0].kids.items():
            visits[it.t, j] += it.nodes[x].V
            wins[it.t, j] += it.nodes[x].W
    return (visits, wins, totals, items) if trace else (visits, wins, totals)


def choose(visits, wins, n, off, ids):
    """int32 [T]: the canonical id at the first maximum of wins / visits over the visited entries of [0 .. n[t]), compared
    exactly in integers, -1 where nothing was visited (ddz_search_choose)"""
    out = np.full(len(n), -1, np.int32)
    for t in range(len(n)):
        best = -1
        for j in range(int(n[t])):
            v, w = int(visits[t, j]), int(wins[t, j])
            if v > 0 and (best < 0 or w * int(visits[t, best]) > int(wins[t, best]) * v):
                best = j
        if best >= 0:
            out[t] = ids[off[t] + best]
    return out
