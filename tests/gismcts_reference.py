"""Search spec v4 (guided ISMCTS) restated on the CPU oracle: what ddz_gismcts_open / _step / _close must leave,
independent of the engine.  numpy and the oracle module (handed in) only; the manner is ismcts_reference.py's (the tree, the
worlds, the descent) crossed with guided_reference.py's (the launches, the unit, the leaf value).

Every (table t, tree c) item owns ONE tree of Python records and one slot of ONE OracleEnv; launch i runs iteration i of every
item in lock-step on world k = c * budget + i of playout spec v2: the slot is set to the root with that world as the opponents'
hands, then legal() -> one move per item (the selected child's index of the list or the expansion index) -> step(STEP_CHOICE,
no auto-reset), until every item has scored or waits for a value.
  node       spec v2's: identified by (parent, canonical id of the move into it): kids {id: node}, V, W in 1024ths, the
             availability count A, terminal, winner
  descent    spec v2's, word for word: L = the list of the state in this world, U = the entries of L without a child; the
             existing children in L get A += 1; U not empty: create the ((draw_e * |U|) >> 32)-th entry of U with A = 1
             (draw_e: domain 6 on (gid, c << 16 | i)); otherwise select among the children in L on the counts of before, ties
             to the lowest index of L
  selection  value = ((float)W / (float)V) * 2^-10 + c * sqrt((2 * LN[A]) / V) in np.float32, one rounding per operation
             (guided_reference.value with the child's own A for N); "sides" away from the root's side counts V * 1024 - W
  expansion  the move empties a hand: a terminal child, ONE if the winner is on the root actor's side, else 0.  Otherwise a
             PENDING LEAF: its row is the slot's 176 bytes (the opponents' hands are this iteration's world), and the
             evaluator's value v (clamped into [0, ONE]) scores v where the leaf's actor is on the root actor's side, else
             ONE - v.  There is no playout and no playout draw
  evaluator  a callable (leaf_rows uint8 [T * trees, 11, 16], need int32 [T * trees], i) -> integers [T * trees]: the chance in
             1024ths that the side of each leaf's ACTOR wins; entries with need = 0 are not read
  launches   [(leaf_rows, need)] per iteration: an item without a pending leaf has an all-zero row and need 0
The backup of launch i's leaves stands ahead of launch i + 1's descent (or in close): here it follows the evaluator at once.
gismcts(trace=True) also says what every iteration walked through: the tests' coverage conditions read it."""
import numpy as np

import constructed_states as cs
import guided_reference as gr
import ismcts_reference as ir
import playout_hidden_reference as phr
import playout_reference as pr
import search_reference as sr

ROW, NFIELDS, F_META = pr.ROW, pr.NFIELDS, pr.F_META
STRIDE = pr.STRIDE
ONE = gr.ONE                   # DDZ_GUIDED_ONE
MAX_DEPTH, MAX_BUDGET = sr.MAX_DEPTH, sr.MAX_BUDGET
value, choose = gr.value, sr.choose
Node, Item = ir.Node, ir.Item


def select(ids, node, nodes, mode, own, c):
    """(index of L, values float32 [len L], took the maximum, tied) where every entry of L = ids has a child"""
    vals = np.empty(len(ids), np.float32)
    for j, a in enumerate(ids):
        k = nodes[node.kids[int(a)]]
        assert 1 <= k.V <= k.A <= MAX_BUDGET and 0 <= k.W <= k.V * ONE
        w = k.W if (own or mode == "reference") else k.V * ONE - k.W
        vals[j] = value(w, k.V, k.A, c)
    take_max = own or mode == "sides"
    best = vals.max() if take_max else vals.min()
    at = np.flatnonzero(vals == best)
    return int(at[0]), vals, take_max, len(at) > 1


def gismcts(oracle, states, budget, evaluator, trees=1, mode="reference", c=0.7, seed=0, gid_base=0, salt=0, roles=0b111,
            stride=STRIDE, trace=False):
    """-> (visits int32 [T, stride], wins int32 [T, stride] in 1024ths, totals int64 [4], launches) of search spec v4 for
    `states` uint8 [T, 11, 16]; with trace=True -> (..., launches, items): items[k].iters[i] = {"path": node numbers from the
    root, "choices": the indices of L applied from the root, "sel": [(depth, node, index of L, took the max, tied, values,
    children the node owned)], "expand": (node, index of L, len L, |U|, the node had been fully expanded before) or None,
    "missing": descent steps at which an existing child's move was not in L, "terminal": the path ended in a terminal node
    that existed before, "pending": the iteration waited for a value, "own": the leaf's actor is on the root actor's side,
    "value": the clamped value, "score", "moves", "winner", "world": the opponents' rows uint8 [2, 16]}, items[k].nodes"""
    assert mode in ("reference", "sides") and 1 <= budget <= MAX_BUDGET and c >= 0 and budget * trees * ONE < 2 ** 31
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
    launches = []
    if not items:
        launches = [(np.zeros((T * trees, NFIELDS, ROW), np.uint8), np.zeros(T * trees, np.int32)) for _ in range(budget)]
        return (visits, wins, totals, launches, items) if trace else (visits, wins, totals, launches)
    I = len(items)
    env = oracle.OracleEnv(I, seed=seed, gid_base=gid_base)
    st = env.state.reshape(I, NFIELDS, ROW)
    m = env.field(F_META)
    gid = np.array([int(gid_base) + it.t for it in items], np.uint64)
    tree = np.array([it.c for it in items], np.int64)
    slot = np.array([it.t * trees + it.c for it in items])
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    DESCEND, ARRIVE, OVER = 0, 1, 2
    for i in range(budget):
        for k, it in enumerate(items):
            st[k] = phr.with_world(states[it.t], W[it.t, it.c * budget + i])
        ctr2 = (tree << 16) | i
        draw_e = cs.philox4x32_10(gid, gid >> np.uint64(32), ctr2, np.full(I, 6 << 16), *key)[0]
        phase = np.full(I, DESCEND)
        cur = [0] * I
        path = [[0] for _ in range(I)]
        made = [None] * I
        moves = np.zeros(I, np.int64)
        pending = np.zeros(I, bool)
        rec = [{"path": path[k], "choices": [], "sel": [], "expand": None, "missing": 0, "terminal": False, "pending": False,
                "own": None, "value": None, "score": 0, "moves": 0, "winner": -1, "world": W[it.t, it.c * budget + i].copy()}
               for k, it in enumerate(items)]
        leaf_rows = np.zeros((T * trees, NFIELDS, ROW), np.uint8)
        need = np.zeros(T * trees, np.int32)
        while (phase != OVER).any():
            off, _, ids = env.legal()
            A = np.diff(off).astype(np.int64)
            done = m[:, pr.M_DONE] == 1
            sel = np.full(I, -1, np.int32)
            for k in np.flatnonzero(phase == ARRIVE):       # the state behind the new child's move
                child, made[k] = made[k], None
                if done[k]:
                    child.terminal = True
                    assert int(m[k, pr.M_WINNER]) == child.winner
                else:
                    child.winner = -1
                    pending[k] = True
                    leaf_rows[slot[k]] = st[k]
                    need[slot[k]] = 1
                phase[k] = OVER
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
                    sel[k], phase[k] = j, ARRIVE
                    totals[3] += 1
                else:
                    node.full = True
                    own = sr._own(mode, role, it.root_role)
                    j, vals, took_max, tied = select(L, node, it.nodes, mode, own, c)
                    rec[k]["sel"].append((node.depth, cur[k], j, took_max, tied, vals, len(node.kids)))
                    for a in L:
                        it.nodes[node.kids[a]].A += 1
                    cur[k] = node.kids[L[j]]
                    path[k].append(cur[k])
                    sel[k] = j
                rec[k]["choices"].append(int(sel[k]))
            act = np.flatnonzero(sel >= 0)
            if len(act) == 0:
                continue
            _, _, illegal, _ = env.step(pr.STEP_CHOICE, sel, auto_reset=False)
            assert not illegal[act].any()
            moves[act] += 1
        launches.append((leaf_rows, need))
        vals = np.asarray(evaluator(leaf_rows.copy(), need.copy(), i)).reshape(-1) if need.any() else np.zeros(T * trees, np.int64)
        done = m[:, pr.M_DONE] == 1
        for k, it in enumerate(items):
            if pending[k]:
                v = min(max(int(vals[slot[k]]), 0), ONE)
                own = (int(m[k, pr.M_ROLE]) == 1) == (it.root_role == 1)
                score, winner = (v if own else ONE - v), -1
                rec[k]["pending"], rec[k]["own"], rec[k]["value"] = True, own, v
            else:
                winner = int(m[k, pr.M_WINNER]) if done[k] else -1
                score = ONE if (winner >= 0 and ((winner == 1) == (it.root_role == 1))) else 0
                totals[2] += winner < 0
            nodes = [it.nodes[x] for x in path[k]]
            if rec[k]["expand"] is not None:
                nodes.append(it.nodes[-1])
            for nd in nodes:
                nd.V += 1
                nd.W += score
            rec[k]["moves"], rec[k]["winner"], rec[k]["score"] = int(moves[k]), winner, score
            if trace:
                it.iters.append(rec[k])
        totals[0] += int(moves.sum())
        totals[1] += I
    for it in items:
        L = [int(a) for a in ids_root[off_root[it.t]:off_root[it.t + 1]]]
        for a, x in it.nodes[0].kids.items():
            visits[it.t, L.index(a)] += it.nodes[x].V
            wins[it.t, L.index(a)] += it.nodes[x].W
    return (visits, wins, totals, launches, items) if trace else (visits, wins, totals, launches)
