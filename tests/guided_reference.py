"""Search spec v3 (guided UCT) restated on the CPU oracle: what ddz_guided_open / _step / _close must leave,
independent of the engine.  numpy, math and the oracle module (handed in) only; the manner is search_reference.py's.

Every (table t, tree c) item owns one slot of ONE OracleEnv and a tree of Python records; launch i runs iteration i of every
item in lock-step: every slot is set back to its root, then legal() -> one move per item (the selected child's list index or
the expansion index) -> step(STEP_CHOICE, no auto-reset), until every item has scored or waits for a value.
  unit       ONE = 1024: W counts 1024ths, V visits
  selection  value = ((float)W / (float)V) * 2^-10 + c * sqrt((2 * LN[N]) / V) in np.float32, one rounding per operation;
             "sides" away from the root's side counts V * 1024 - W; modes, ties and LN are spec v1's
  expansion  spec v1's draw (domain 6) and pick.  The move empties a hand: a terminal child, ONE if the winner is on the root
             actor's side, else 0.  Otherwise a PENDING LEAF: n = the size of its state's list, its row is the slot's 176
             bytes, and the evaluator's value v (clamped into [0, ONE]) scores v where the leaf's actor is on the root
             actor's side, else ONE - v
  evaluator  a callable (leaf_rows uint8 [T * trees, 11, 16], need int32 [T * trees], i) -> integers [T * trees]: the chance
             in 1024ths that the side of each leaf's ACTOR wins; entries with need = 0 are not read
  launches   [(leaf_rows, need)] per iteration: an item without a pending leaf has an all-zero row and need 0
guided(trace=True) also says what every iteration walked through: the tests' coverage conditions read it."""
import numpy as np

import constructed_states as cs
import playout_hidden_reference as phr
import playout_reference as pr
import search_reference as sr

ROW, NFIELDS, F_META = pr.ROW, pr.NFIELDS, pr.F_META
STRIDE = pr.STRIDE
ONE = 1024                     # DDZ_GUIDED_ONE
MAX_DEPTH, MAX_BUDGET, LN = sr.MAX_DEPTH, sr.MAX_BUDGET, sr.LN
F32 = np.float32


def value(W, V, N, c):
    """the fp32 value of a child with (V, W in 1024ths) under a parent with N visits: spec v1's operations and one exact scaling"""
    fv = F32(V)
    mean = (F32(W) / fv) * F32(2.0 ** -10)
    q = (F32(2.0) * LN[N]) / fv
    return mean + F32(c) * np.sqrt(q)


def select(node, nodes, mode, own, c):
    """(list index, values float32 [n], took the maximum, tied) at a fully expanded node"""
    vals = np.empty(node.n, np.float32)
    for j in range(node.n):
        k = nodes[node.kids[j]]
        w = k.W if (own or mode == "reference") else k.V * ONE - k.W
        vals[j] = value(w, k.V, node.V, c)
    take_max = own or mode == "sides"
    best = vals.max() if take_max else vals.min()
    at = np.flatnonzero(vals == best)
    return int(at[0]), vals, take_max, len(at) > 1


def guided(oracle, states, budget, evaluator, trees=1, mode="reference", c=0.7, seed=0, gid_base=0, salt=0, hidden=False,
           roles=0b111, stride=STRIDE, trace=False):
    """-> (visits int32 [T, stride], wins int32 [T, stride] in 1024ths, totals int64 [4], launches) of search spec v3 for
    `states` uint8 [T, 11, 16]; with trace=True -> (..., launches, items): items[k].iters[i] = {"path": node numbers from the
    root, "choices": the list indices applied from the root, "sel": [(depth, node, list index, took the max, tied, values)],
    "expand": (node, list index, n of the node) or None, "expand_id": the canonical id of its move (beside "expand"), "terminal": the path ended in a terminal node that existed before,
    "pending": the iteration waited for a value, "own": the leaf's actor is on the root actor's side, "value": the clamped
    value, "score", "moves", "winner"}, items[k].nodes"""
    assert mode in ("reference", "sides") and 1 <= budget <= MAX_BUDGET and c >= 0 and budget * trees * ONE < 2 ** 31
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
            it = sr.Item(int(t), k, root, role, budget)
            it.nodes[0].n = int(n_root[t])
            items.append(it)
    launches = []
    if not items:
        zero = (np.zeros((T * trees, NFIELDS, ROW), np.uint8), np.zeros(T * trees, np.int32))
        launches = [(zero[0].copy(), zero[1].copy()) for _ in range(budget)]
        return (visits, wins, totals, launches, items) if trace else (visits, wins, totals, launches)
    I = len(items)
    env = oracle.OracleEnv(I, seed=seed, gid_base=gid_base)
    st = env.state.reshape(I, NFIELDS, ROW)
    m = env.field(F_META)
    roots = np.stack([it.root for it in items])
    gid = np.array([int(gid_base) + it.t for it in items], np.uint64)
    tree = np.array([it.c for it in items], np.int64)
    slot = np.array([it.t * trees + it.c for it in items])
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    DESCEND, ARRIVE, OVER = 0, 1, 2
    for i in range(budget):
        st[:] = roots
        ctr2 = (tree << 16) | i
        draw_e = cs.philox4x32_10(gid, gid >> np.uint64(32), ctr2, np.full(I, 6 << 16), *key)[0]
        phase = np.full(I, DESCEND)
        cur = [0] * I
        path = [[0] for _ in range(I)]
        made = [None] * I
        moves = np.zeros(I, np.int64)
        pending = np.zeros(I, bool)
        rec = [{"path": path[k], "choices": [], "sel": [], "expand": None, "terminal": False, "pending": False, "own": None,
                "value": None, "score": 0, "moves": 0, "winner": -1} for k in range(I)]
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
                    child.terminal, child.n = True, 0
                    assert int(m[k, pr.M_WINNER]) == child.winner
                else:
                    child.n, child.winner = int(A[k]), -1
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
                assert not done[k] and node.n == A[k]
                if node.n == 0 or node.depth == MAX_DEPTH:
                    phase[k] = OVER          # outside the domain: unfinished
                    continue
                role = int(m[k, pr.M_ROLE])
                if len(node.kids) < node.n:
                    untried = [j for j in range(node.n) if j not in node.kids]
                    j = untried[(int(draw_e[k]) * len(untried)) >> 32]
                    child = sr.Node(node.depth + 1)
                    node.kids[j] = len(it.nodes)
                    it.probe.insert(cur[k], j)
                    rec[k]["expand"] = (cur[k], j, node.n)
                    rec[k]["expand_id"] = int(ids[off[k] + j])
                    it.nodes.append(child)
                    made[k] = child
                    child.winner = role      # (used if the move empties the hand)
                    sel[k], phase[k] = j, ARRIVE
                    totals[3] += 1
                else:
                    own = sr._own(mode, role, it.root_role)
                    j, vals, took_max, tied = select(node, it.nodes, mode, own, c)
                    rec[k]["sel"].append((node.depth, cur[k], j, took_max, tied, vals))
                    cur[k] = node.kids[j]
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
        for j, x in it.nodes[0].kids.items():
            visits[it.t, j] += it.nodes[x].V
            wins[it.t, j] += it.nodes[x].W
    return (visits, wins, totals, launches, items) if trace else (visits, wins, totals, launches)


def v1_playout_leaf(oracle, trees, seed=0, gid_base=0, salt=0, max_plies=pr.MAX_PLIES):
    """the evaluator that makes spec v3 spec v1: spec v1's playout from the leaf -- index (draw * A) >> 32, draw =
    philox((gid_lo, gid_hi, c << 16 | i, 7 << 16 | ply), key).x, at most max_plies moves -- scored ONE if the winner is on
    the LEAF actor's side, else 0.  A playout that does not finish has no such score (spec v1 gives it 0 from the ROOT's
    side): the callers' cases are inside the domain, where every playout ends, and this asserts it."""
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]

    def evaluator(rows, need, i):
        at = np.flatnonzero(need)
        out = np.zeros(len(need), np.int64)
        env = oracle.OracleEnv(len(at), seed=seed, gid_base=gid_base)
        env.state.reshape(len(at), NFIELDS, ROW)[:] = rows[at]
        m = env.field(F_META)
        actor = m[:, pr.M_ROLE].astype(np.int64).copy()
        gid = (np.uint64(int(gid_base)) + (at // trees).astype(np.uint64))
        ctr2 = ((at % trees).astype(np.int64) << 16) | i
        for _ in range(max_plies):
            off, _, _ = env.legal()
            A = np.diff(off).astype(np.int64)
            go = np.flatnonzero((m[:, pr.M_DONE] != 1) & (A > 0))
            if len(go) == 0:
                break
            ply = m[:, pr.M_PLY].astype(np.int64) | (m[:, pr.M_PLY + 1].astype(np.int64) << 8)
            d = cs.philox4x32_10(gid[go], gid[go] >> np.uint64(32), ctr2[go], (7 << 16) | ply[go], *key)[0]
            sel = np.full(len(at), -1, np.int32)
            sel[go] = ((d * A[go].astype(np.uint64)) >> np.uint64(32)).astype(np.int32)
            env.step(pr.STEP_CHOICE, sel, auto_reset=False)
        assert (m[:, pr.M_DONE] == 1).all(), "a playout did not finish: outside the domain of the v3 = v1 check"
        winner = m[:, pr.M_WINNER].astype(np.int64)
        out[at] = np.where((winner == 1) == (actor == 1), ONE, 0)
        return out

    return evaluator


def hash_leaf(rows, need, i):
    """a deterministic integer hash of each leaf row into [-50, 1100]: beyond both ends of [0, ONE], so the clamp, 0 and ONE
    are all exercised.  FNV-1a over the 176 bytes in 64-bit integers; half of the rows (by the hash's top bit) get any
    integer of the range, the other half a multiple of 50, so that siblings meet with equal scores and selection has ties
    to break."""
    rows = np.asarray(rows, np.uint8).reshape(len(need), -1).astype(np.uint64)
    h = np.full(len(need), 0xCBF29CE484222325, np.uint64)
    with np.errstate(over="ignore"):
        for b in range(rows.shape[1]):
            h = (h ^ rows[:, b]) * np.uint64(0x100000001B3)
    fine = ((h >> np.uint64(16)) % np.uint64(1151)).astype(np.int64) - 50
    coarse = ((h >> np.uint64(40)) % np.uint64(24)).astype(np.int64) * 50 - 50
    return np.where((h >> np.uint64(63)) == 1, coarse, fine)


def playout_leaf(oracle, K, seed=0, salt=0):
    """engine.PlayoutLeaf(K) restated: the leaf rows as tables 0 .. of a scratch environment with the searched one's seed and
    table_id_base 0, playout spec v1 with K playouts per move there, value = (max_j wins_j * 1024) // K"""
    def evaluator(rows, need, i):
        w, _ = pr.playouts(oracle, rows, K, seed=seed, gid_base=0, salt=salt)[:2]
        return (w.max(1).astype(np.int64) * ONE) // K

    return evaluator
