"""Search spec v5 (guided PUCT) restated on the CPU oracle: what ddz_puct_open / _step / _close must leave,
independent of the engine.  numpy and the oracle module (handed in) only; the manner is guided_reference.py's.

Every (table t, tree c) item owns one slot of ONE OracleEnv, a tree of Python records and an integer prior pool (a uint8
array of `pool` bytes and a fill mark); launch i runs iteration i of every item in lock-step.
  unit       ONE = 1024: W counts 1024ths, V visits; always the "sides" rule: a node's actor maximises its own side's mean
  iteration 0  descends nowhere: node 0 waits with the root's own row (hidden: on the tree's world), need = 1
  selection  at a node with n entries and N = V visits, over EVERY list index j, in np.float32, one rounding per operation:
               mean_j = (Wside_j / V_j) * 2^-10 where child j exists, else the node's own (Wside / N) * 2^-10
               p_j    = w_j / S, or 1 / n where the node has no stored run or S = 0
               value_j = mean_j + ((c * p_j) * sqrt(N)) / (1 + V_j);   the maximum, ties to the lowest index
             Wside = W where the node's actor is on the root actor's side, else V * 1024 - W
  expansion  the selected index has no child: the child is made.  The move empties a hand: terminal, ONE if the winner is on
             the root actor's side, else 0, backed up at once, no run.  Otherwise it waits: n = the size of its list, its row
             is the slot's 176 bytes
  backup     of a waiting node with the evaluator's (value, priors): v clamped into [0, ONE] scores v where the node's actor
             is on the root actor's side, else ONE - v; V += 1, W += score on the path and the node; then the node's n
             weights priors[slot, 0 .. n) go to the pool at the fill mark, which moves on by n rounded up to RUN_ALIGN; a run
             that does not fit is not stored (uniform; totals[4] += 1).  n = 0: no run, not counted
  evaluator  a callable (leaf_rows uint8 [T * trees, 11, 16], need int32 [T * trees], i) -> (values [T * trees], priors
             uint8 [T * trees, stride]); entries with need = 0 and weights at or beyond n are not read
puct(trace=True) also says what every iteration walked through: the tests' coverage conditions read it."""
import numpy as np

import guided_reference as gr
import playout_hidden_reference as phr
import playout_reference as pr
import search_reference as sr

ROW, NFIELDS, F_META = pr.ROW, pr.NFIELDS, pr.F_META
STRIDE = pr.STRIDE
ONE = gr.ONE
MAX_DEPTH, MAX_BUDGET = sr.MAX_DEPTH, sr.MAX_BUDGET
RUN_ALIGN = 4                  # PUCT_RUN_ALIGN
POOL_MAX = 1 << 24
F32 = np.float32


def default_pool(budget):
    """64 bytes a node, rounded up to 16"""
    return (64 * int(budget) + 15) & ~15


class Node(sr.Node):
    __slots__ = ("off", "S")

    def __init__(self, depth):
        super().__init__(depth)
        self.off, self.S = None, 0


class Item(sr.Item):
    def __init__(self, t, c, root, root_role, budget, pool):
        super().__init__(t, c, root, root_role, budget)
        self.nodes = [Node(0)]
        self.pool = np.zeros(pool, np.uint8)
        self.used = 0
        self.fallback = 0


def values(node, nodes, pool, own, c):
    """float32 [n]: value_j of every list index of an evaluated node, and the int64 [n] visits of its children"""
    n, N = node.n, node.V
    assert n > 0 and N >= 1
    V, W = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j, x in node.kids.items():
        V[j], W[j] = nodes[x].V, nodes[x].W
    side = W if own else V * ONE - W
    side0 = node.W if own else N * ONE - node.W
    mean0 = (F32(side0) / F32(N)) * F32(2.0 ** -10)
    with np.errstate(all="ignore"):
        mean = np.where(V > 0, (side.astype(F32) / V.astype(F32)) * F32(2.0 ** -10), mean0).astype(F32)
    if node.off is not None and node.S > 0:
        p = pool[node.off:node.off + n].astype(F32) / F32(node.S)
    else:
        p = np.full(n, F32(1.0) / F32(n), F32)
    u = ((F32(c) * p) * np.sqrt(F32(N))) / (1 + V).astype(F32)
    out = mean + u
    assert out.dtype == F32
    return out, V


def select(node, nodes, pool, own, c):
    """(list index, values float32 [n], tied) at an evaluated node: the first maximum"""
    vals, _ = values(node, nodes, pool, own, c)
    at = np.flatnonzero(vals == vals.max())
    return int(at[0]), vals, len(at) > 1


def store_priors(it, node, w):
    """the run of `node` (n weights, uint8) goes to the item's pool, or the node falls back to uniform"""
    n = node.n
    if n <= 0:
        return
    run = (n + RUN_ALIGN - 1) & ~(RUN_ALIGN - 1)
    if run <= len(it.pool) - it.used:
        node.off, it.used = it.used, it.used + run
        it.pool[node.off:node.off + n] = w[:n]
        node.S = int(w[:n].astype(np.int64).sum())
    else:
        it.fallback += 1


def puct(oracle, states, budget, leaf, trees=1, c=1.25, seed=0, gid_base=0, salt=0, hidden=False, roles=0b111, stride=STRIDE,
         pool=None, trace=False):
    """-> (visits int32 [T, stride], wins int32 [T, stride] in 1024ths, totals int64 [5], launches) of search spec v5 for
    `states` uint8 [T, 11, 16]; with trace=True -> (..., launches, items): items[k].iters[i] = {"path": node numbers from the
    root, "choices": the list indices applied from the root, "sel": [(depth, node, list index, the index had a child, children
    of the node, tied, values)], "expand": (node, list index, n of the node) or None, "root": iteration 0, "terminal": the path
    ended in a terminal node that existed before, "pending": the iteration waited for a value, "own": the waiting node's actor
    is on the root actor's side, "value": the clamped value, "S": the weight sum stored (None: no run), "fallback", "score",
    "moves", "winner"}, items[k].nodes, .pool, .used, .fallback"""
    pool = default_pool(budget) if pool is None else int(pool)
    assert 1 <= budget <= MAX_BUDGET and c >= 0 and budget * trees * ONE < 2 ** 31 and 16 <= pool <= POOL_MAX and pool % 16 == 0
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T = len(states)
    visits, wins = np.zeros((T, stride), np.int32), np.zeros((T, stride), np.int32)
    totals = np.zeros(5, np.int64)
    n_root, _, _ = pr.root_lists(oracle, states, seed, gid_base)
    if hidden:
        W, part, _ = phr.worlds(oracle, states, trees, seed, gid_base, salt, roles)
        n_root = np.where(part, n_root, 0)
    items = []
    for t in np.flatnonzero(n_root > 0):
        role = int(states[t, F_META, pr.M_ROLE]) % 3
        for k in range(trees):
            root = phr.with_world(states[t], W[t, k]) if hidden else states[t].copy()
            it = Item(int(t), k, root, role, budget, pool)
            it.nodes[0].n = int(n_root[t])
            items.append(it)
    launches = []
    if not items:
        launches = [(np.zeros((T * trees, NFIELDS, ROW), np.uint8), np.zeros(T * trees, np.int32)) for _ in range(budget)]
        return (visits, wins, totals, launches, items) if trace else (visits, wins, totals, launches)
    I = len(items)
    env = oracle.OracleEnv(I, seed=seed, gid_base=gid_base)
    st = env.state.reshape(I, NFIELDS, ROW)
    m = env.field(F_META)
    roots = np.stack([it.root for it in items])
    slot = np.array([it.t * trees + it.c for it in items])
    DESCEND, ARRIVE, OVER = 0, 1, 2
    for i in range(budget):
        st[:] = roots
        phase = np.full(I, DESCEND if i else OVER)
        cur = [0] * I
        path = [[0] for _ in range(I)]
        made = [None] * I
        waiting = [None] * I          # the node that waits for its value and priors
        moves = np.zeros(I, np.int64)
        rec = [{"path": path[k], "choices": [], "sel": [], "expand": None, "root": i == 0, "terminal": False, "pending": False,
                "own": None, "value": None, "S": None, "fallback": False, "score": 0, "moves": 0, "winner": -1} for k in range(I)]
        leaf_rows = np.zeros((T * trees, NFIELDS, ROW), np.uint8)
        need = np.zeros(T * trees, np.int32)
        if i == 0:                    # iteration 0 evaluates the root
            for k, it in enumerate(items):
                waiting[k] = it.nodes[0]
                leaf_rows[slot[k]] = st[k]
                need[slot[k]] = 1
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
                    waiting[k] = child
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
                own = (role == 1) == (it.root_role == 1)
                j, vals, tied = select(node, it.nodes, it.pool, own, c)
                rec[k]["sel"].append((node.depth, cur[k], j, j in node.kids, len(node.kids), tied, vals))
                if j in node.kids:
                    cur[k] = node.kids[j]
                    path[k].append(cur[k])
                else:
                    child = Node(node.depth + 1)
                    node.kids[j] = len(it.nodes)
                    it.probe.insert(cur[k], j)
                    rec[k]["expand"] = (cur[k], j, node.n)
                    rec[k]["expand_id"] = int(ids[off[k] + j])
                    it.nodes.append(child)
                    made[k] = child
                    child.winner = role      # (used if the move empties the hand)
                    phase[k] = ARRIVE
                    totals[3] += 1
                sel[k] = j
                rec[k]["choices"].append(j)
            act = np.flatnonzero(sel >= 0)
            if len(act) == 0:
                continue
            _, _, illegal, _ = env.step(pr.STEP_CHOICE, sel, auto_reset=False)
            assert not illegal[act].any()
            moves[act] += 1
        launches.append((leaf_rows, need))
        if need.any():
            vals, pri = leaf(leaf_rows.copy(), need.copy(), i)
            vals, pri = np.asarray(vals).reshape(-1), np.asarray(pri, np.uint8).reshape(T * trees, -1)
        done = m[:, pr.M_DONE] == 1
        for k, it in enumerate(items):
            nodes = [it.nodes[x] for x in path[k]]
            if waiting[k] is not None:
                v = min(max(int(vals[slot[k]]), 0), ONE)
                own = (int(m[k, pr.M_ROLE]) == 1) == (it.root_role == 1)
                score, winner = (v if own else ONE - v), -1
                before = it.fallback
                store_priors(it, waiting[k], pri[slot[k]])
                rec[k].update(pending=True, own=own, value=v, fallback=it.fallback > before,
                              S=None if waiting[k].off is None else waiting[k].S)
                if i > 0:
                    nodes.append(waiting[k])
            else:
                winner = int(m[k, pr.M_WINNER]) if done[k] else -1
                score = ONE if (winner >= 0 and ((winner == 1) == (it.root_role == 1))) else 0
                totals[2] += winner < 0
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
        totals[4] += it.fallback
        for j, x in it.nodes[0].kids.items():
            visits[it.t, j] += it.nodes[x].V
            wins[it.t, j] += it.nodes[x].W
    return (visits, wins, totals, launches, items) if trace else (visits, wins, totals, launches)


def playout_leaf(oracle, K, seed=0, salt=0, stride=STRIDE):
    """engine.PlayoutLeaf(K) on a search with priors, restated: playout spec v1 with K playouts per move on the leaf rows as
    tables 0 .. of a scratch environment, value = (max_j wins_j * 1024) // K, w_j = 1 + (254 * wins_j) // K"""
    def evaluator(rows, need, i):
        w = pr.playouts(oracle, rows, K, seed=seed, gid_base=0, salt=salt)[0].astype(np.int64)
        return (w.max(1) * ONE) // K, (1 + (254 * w) // K).astype(np.uint8)

    return evaluator
