"""Search spec v2 (ISMCTS) restated on the CPU oracle: what ddz_ismcts must count, independent of the engine.
numpy, the oracle module (handed in), search_reference (the fp32 value, LN, choose) and playout_hidden_reference (the worlds).

Single-observer information-set MCTS (Whitehouse, Powley, Cowling, CIG 2011; Cowling, Powley, Whitehouse, TCIAIG 2012): every
(table t, tree c) item owns ONE tree; iteration i plays on world k = c * budget + i of playout spec v2, and every step of the
descent sees only the moves legal in that world.
  node       identified by (parent, canonical id of the move into it): kids {id: node}, V, W, the availability count A (how many
             iterations met the node's move in their list while the node existed, its creation included), terminal, winner
  descent    L = the list of the state in this world (ascending id); U = the entries of L without a child.  U not empty: create
             the ((draw_e * |U|) >> 32)-th entry of U with A = 1, the existing children in L get A += 1, playout.  Otherwise
             select among the children in L with value = W/V + c * sqrt((2 * LN[A]) / V), the child's own A (search_reference.
             value with A for N), ties to the lowest index of L, then every child in L gets A += 1
  the rest   draws (domains 6 and 7 on (gid, c << 16 | i, ..)), playout, score, backup, totals and root outputs are spec v1's
ismcts(trace=True) also says what every iteration walked through: the tests' coverage conditions read it."""
import numpy as np

import constructed_states as cs
import playout_hidden_reference as phr
import playout_reference as pr
import search_reference as sr

ROW, NFIELDS, F_META = pr.ROW, pr.NFIELDS, pr.F_META
STRIDE = pr.STRIDE
MAX_PLIES, MAX_DEPTH, MAX_BUDGET = sr.MAX_PLIES, sr.MAX_DEPTH, sr.MAX_BUDGET
choose = sr.choose


class Node:
    __slots__ = ("kids", "V", "W", "A", "terminal", "winner", "depth", "full")

    def __init__(self, depth):
        self.kids, self.V, self.W, self.A, self.terminal, self.winner, self.depth = {}, 0, 0, 1, False, -1, depth
        self.full = False            # trace only: some world's list found every entry with a child here


class Item:
    def __init__(self, t, c, root_role):
        self.t, self.c, self.root_role = t, c, root_role
        self.nodes = [Node(0)]
        self.iters = []              # trace: one dict per iteration


def select(ids, node, nodes, mode, own, c):
    """(index of L, values float32 [len L], took the maximum, tied) where every entry of L = ids has a child"""
    vals = np.empty(len(ids), np.float32)
    for j, a in enumerate(ids):
        k = nodes[node.kids[int(a)]]
        assert 1 <= k.V <= k.A <= MAX_BUDGET
        w = k.W if (own or mode == "reference") else k.V - k.W
        vals[j] = sr.value(w, k.V, k.A, c)
    take_max = own or mode == "sides"
    best = vals.max() if take_max else vals.min()
    at = np.flatnonzero(vals == best)
    return int(at[0]), vals, take_max, len(at) > 1


def ismcts(oracle, states, budget, trees=1, mode="reference", c=0.7, seed=0, gid_base=0, salt=0, roles=0b111, stride=STRIDE,
           max_plies=MAX_PLIES, trace=False):
    """-> (visits int32 [T, stride], wins int32 [T, stride], totals int64 [4]) of search spec v2 for `states` uint8 [T, 11, 16];
    with trace=True -> (visits, wins, totals, items): items[k].iters[i] = {"path": node numbers from the root, "sel": [(depth,
    node, index of L, took the max, tied, values)], "expand": (node, index of L, len L, |U|, the node had been fully expanded
    before) or None, "missing": descent steps at which an existing child's move was not in L, "terminal": the path ended in a
    terminal node that existed before, "moves", "winner"}, items[k].nodes"""
    assert mode in ("reference", "sides") and 1 <= budget <= MAX_BUDGET and c >= 0
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T = len(states)
    visits, wins = np.zeros((T, stride), np.int32), np.zeros((T, stride), np.int32)
    totals = np.zeros(4, np.int64)
    n_root, off_root, ids_root = pr.root_lists(oracle, states, seed, gid_base)
    W, part, _ = phr.worlds(oracle, states, trees * budget, seed, gid_base, salt, roles)
    n_root = np.where(part, n_root, 0)
    items = []
    for t in np.flatnonzero(n_root > 0):
        role = int(states[t, F_META, pr.M_ROLE]) % 3
        items += [Item(int(t), k, role) for k in range(trees)]
    if not items:
        return (visits, wins, totals, items) if trace else (visits, wins, totals)
    I = len(items)
    env = oracle.OracleEnv(I, seed=seed, gid_base=gid_base)
    st = env.state.reshape(I, NFIELDS, ROW)
    m = env.field(F_META)
    gid = np.array([int(gid_base) + it.t for it in items], np.uint64)
    tree = np.array([it.c for it in items], np.int64)
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    DESCEND, PLAYOUT, OVER = 0, 1, 2
    for i in range(budget):
        for k, it in enumerate(items):
            st[k] = phr.with_world(states[it.t], W[it.t, it.c * budget + i])
        ctr2 = (tree << 16) | i
        draw_e = cs.philox4x32_10(gid, gid >> np.uint64(32), ctr2, np.full(I, 6 << 16), *key)[0]
        phase = np.full(I, DESCEND)
        cur = [0] * I
        path = [[0] for _ in range(I)]
        made = [None] * I            # the node created by this iteration, waiting to learn whether its move ended the game
        left = np.zeros(I, np.int64)  # playout moves still allowed
        moves = np.zeros(I, np.int64)
        rec = [{"path": path[k], "sel": [], "expand": None, "missing": 0, "terminal": False, "moves": 0, "winner": -1}
               for k in range(I)]
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
                assert not done[k]
                if A[k] == 0 or node.depth == MAX_DEPTH:
                    phase[k] = OVER          # outside the domain: unfinished
                    continue
                L = [int(a) for a in ids[off[k]:off[k + 1]]]
                assert len(set(L)) == len(L) and L == sorted(L)
                if node.depth == 0:          # the root actor's own list is the same in every world
                    assert L == [int(a) for a in ids_root[off_root[it.t]:off_root[it.t + 1]]]
                role = int(m[k, pr.M_ROLE])
                U = [j for j, a in enumerate(L) if a not in node.kids]
                rec[k]["missing"] += any(a not in L for a in node.kids)
                if U:
                    j = U[(int(draw_e[k]) * len(U)) >> 32]
                    for a in L:
                        if a in node.kids:
                            it.nodes[node.kids[a]].A += 1
                    child = Node(node.depth + 1)
                    node.kids[L[j]] = len(it.nodes)
                    rec[k]["expand"] = (cur[k], j, len(L), len(U), node.full)
                    it.nodes.append(child)
                    made[k] = child
                    child.winner = role      # (used if the move empties the hand)
                    sel[k], phase[k], left[k] = j, PLAYOUT, max_plies
                    totals[3] += 1
                else:
                    node.full = True
                    own = sr._own(mode, role, it.root_role)
                    j, vals, took_max, tied = select(L, node, it.nodes, mode, own, c)
                    rec[k]["sel"].append((node.depth, cur[k], j, took_max, tied, vals))
                    for a in L:
                        it.nodes[node.kids[a]].A += 1
                    cur[k] = node.kids[L[j]]
                    path[k].append(cur[k])
                    sel[k] = j
            # the playouts, all at once: the state behind the new child's move, then (draw * A) >> 32
            play = np.flatnonzero((phase == PLAYOUT) & (sel < 0))
            for k in play:
                if made[k] is not None:      # the first state of the playout: a terminal child, or not
                    child, made[k] = made[k], None
                    if done[k]:
                        child.terminal = True
                        assert int(m[k, pr.M_WINNER]) == child.winner
                    else:
                        child.winner = -1
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
        L = [int(a) for a in ids_root[off_root[it.t]:off_root[it.t + 1]]]
        for a, x in it.nodes[0].kids.items():
            visits[it.t, L.index(a)] += it.nodes[x].V
            wins[it.t, L.index(a)] += it.nodes[x].W
    return (visits, wins, totals, items) if trace else (visits, wins, totals)
