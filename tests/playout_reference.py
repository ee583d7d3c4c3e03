"""Playout spec v1 restated on the CPU oracle: what ddz_playout must count, independent of the engine.

Every root state is replicated once per (move index j, playout number k) into ONE OracleEnv; the root moves are applied with
STEP_CHOICE; then, until every copy is done, the loop is legal() -> index from oracle.philox -> step(STEP_CHOICE, no
auto-reset).  Nothing here touches the GPU library; numpy and the oracle module (handed in) only.
  draw  = philox4x32_10((gid_lo, gid_hi, k << 9 | j, 4 << 16 | ply), (seed_lo ^ salt, seed_hi)).x, gid = gid_base + t,
          ply = the u16 ply counter of the state being stepped
  index = (draw * A) >> 32 into the state's legal list of A moves; A = 0 on a running copy stops it (unfinished)
  wins[t][j] = the playouts of move j that ended with a winner on the root actor's side (the lord alone, or either farmer)
  totals = {moves applied (root moves included), playouts run, playouts stopped unfinished, 0}
playouts(trace=True) also says what every playout walked through (class Trace): the tests' coverage conditions read it."""
import numpy as np

ROW, NFIELDS = 16, 11
F_META = 10
M_ROLE, M_DONE, M_WINNER, M_PLY, M_DEALT = 0, 1, 2, 4, 6
STRIDE = 512
MAX_PLIES = 192          # DDZ_PLAYOUT_MAX_PLIES: moves applied per playout at most, the root move included
STEP_CHOICE = 1


def _env(oracle, states, seed, gid_base):
    env = oracle.OracleEnv(len(states), seed=seed, gid_base=gid_base)
    env.state[:] = np.ascontiguousarray(states, np.uint8).reshape(-1)
    return env


def root_lists(oracle, states, seed=0, gid_base=0):
    """(n int64 [T], off, ids): sizes and canonical ids of the oracle's legal lists of `states` (idle tables: empty)"""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    off, _, ids = _env(oracle, states, seed, gid_base).legal()
    return np.diff(off).astype(np.int64), off.copy(), ids.copy()


STEP_DTYPE = np.dtype([("copy", np.int32), ("s", np.int16), ("ply", np.int32), ("A", np.int32), ("index", np.int32),
                       ("id", np.int32), ("beat", np.int32), ("two_passes", np.bool_)])


class Trace:
    """What the playouts of one playouts() call walked through.  Per copy c = (t, j, k), in the order the copies are laid out
    (table, then move, then playout number): t / j / k, moves = moves applied, winner = the winning role or -1.
    steps (STEP_DTYPE, sorted by copy, then s): one entry per applied move -- s = its number within the playout (0 = the root
    move), ply = the u16 ply counter of the state it was applied to, A = the size of that state's legal list, index = the
    picked position, id = the picked canonical action id, beat = the action id to beat (0 = a lead), two_passes = the lead
    follows two passes made INSIDE this playout (a root's own lead is not marked: its recent rows are empty either way).
    beat is not read from the oracle's lists: it is carried from the root's recent rows (envi.py:103-109) through the picked
    ids, and held to the lists by one property, that a list starts with the pass exactly when there is something to beat.
    moves_per_table int64 [T]: the moves applied by all the copies of a table."""

    def __init__(self, t, j, k, moves, winner, steps, T):
        self.t, self.j, self.k, self.moves, self.winner, self.steps = t, j, k, moves, winner, steps
        self.moves_per_table = np.bincount(t, weights=moves, minlength=T).astype(np.int64)
        self._first = np.searchsorted(steps["copy"], np.arange(len(t) + 1))

    def plies(self, c):
        """the per-ply list of copy c: (ply, A, index, id, beat, two_passes) per applied move"""
        return [tuple(x)[2:] for x in self.steps[self._first[c]:self._first[c + 1]].tolist()]

    def records(self):
        """one dict per copy"""
        return [{"t": int(self.t[c]), "j": int(self.j[c]), "k": int(self.k[c]), "moves": int(self.moves[c]),
                 "winner": int(self.winner[c]), "plies": self.plies(c)} for c in range(len(self.t))]


def root_beats(oracle, states):
    """(beat id int64 [T], passes int64 [T]) of envi.py:103-109: the handout of the player before the actor, else of the one
    before that (one pass since), else a lead (0, 0)"""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    beat, passes = np.zeros(len(states), np.int64), np.zeros(len(states), np.int64)
    for t, s in enumerate(states):
        role = int(s[F_META, M_ROLE]) % 3
        for p, r in enumerate(((role + 2) % 3, (role + 1) % 3)):
            row = s[6 + r, :15]
            if row.any():
                beat[t], passes[t] = oracle.lookup(row.astype(np.int8)), p
                assert beat[t] > 0
                break
    return beat, passes


def playouts(oracle, states, n_playouts, seed=0, gid_base=0, salt=0, stride=STRIDE, max_plies=MAX_PLIES, trace=False):
    """-> (wins int32 [T, stride], totals int64 [4]) of playout spec v1 for `states` uint8 [T, 11, 16]; with trace=True
    -> (wins, totals, Trace)"""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T, K = len(states), int(n_playouts)
    wins = np.zeros((T, stride), np.int32)
    totals = np.zeros(4, np.int64)
    n, _, _ = root_lists(oracle, states, seed, gid_base)
    assert n.max(initial=0) <= stride
    # one copy per (t, j, k); idle tables have n = 0 and get none
    tt = np.repeat(np.arange(T), n * K)
    if len(tt) == 0:
        none = np.zeros(0, np.int64)
        return (wins, totals, Trace(none, none, none, none, none, np.zeros(0, STEP_DTYPE), T)) if trace else (wins, totals)
    within = np.arange(len(tt)) - np.repeat(np.cumsum(n * K) - n * K, n * K)
    jj, kk = within // K, within % K
    env = _env(oracle, states[tt], seed, gid_base)
    m = env.field(F_META)
    root_role = m[:, M_ROLE].copy()
    off, _, ids = env.legal()
    if trace:
        steps, moves = [], np.zeros(len(tt), np.int64)
        last, passes = (x[tt] for x in root_beats(oracle, states))

        def record(s, act, sel):
            """the moves sel[act] about to be applied to the copies `act` (off / ids / m: their lists and meta rows now)"""
            e = np.zeros(len(act), STEP_DTYPE)
            e["copy"], e["s"], e["index"] = act, s, sel[act]
            e["ply"] = m[act, M_PLY].astype(np.int64) | (m[act, M_PLY + 1].astype(np.int64) << 8)
            e["A"] = np.diff(off)[act]
            e["id"] = ids[off[:-1][act] + sel[act]]
            lead = (passes[act] >= 2) | (last[act] == 0)
            e["beat"] = np.where(lead, 0, last[act])
            e["two_passes"] = (passes[act] >= 2) & (last[act] > 0)
            assert np.array_equal(ids[off[:-1][act]] == 0, ~lead), "a list starts with the pass <=> there is a move to beat"
            played = e["id"] > 0
            last[act] = np.where(played, e["id"], np.where(lead, 0, last[act]))
            passes[act] = np.where(played, 0, passes[act] + 1)
            moves[act] += 1
            steps.append(e)

        record(0, np.arange(len(tt)), jj)
    _, _, illegal, _ = env.step(STEP_CHOICE, jj.astype(np.int32), auto_reset=False)
    assert not illegal.any()
    totals[0] += len(tt)
    gid = np.uint64(gid_base) + tt.astype(np.uint64)
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    stopped = np.zeros(len(tt), bool)
    for it in range(max_plies - 1):
        off, _, ids = env.legal()
        A = np.diff(off).astype(np.int64)
        stopped |= (m[:, M_DONE] == 0) & (A == 0)
        act = np.flatnonzero((m[:, M_DONE] == 0) & (A > 0))
        if len(act) == 0:
            break
        ply = m[:, M_PLY].astype(np.int64) | (m[:, M_PLY + 1].astype(np.int64) << 8)
        sel = np.full(len(tt), -1, np.int32)
        for c in act:
            g = int(gid[c])
            draw = int(oracle.philox([g & 0xFFFFFFFF, g >> 32, (int(kk[c]) << 9) | int(jj[c]), (4 << 16) | int(ply[c])], key)[0])
            sel[c] = (draw * int(A[c])) >> 32
        if trace:
            record(it + 1, act, sel)
        env.step(STEP_CHOICE, sel, auto_reset=False)
        totals[0] += len(act)
    done = m[:, M_DONE] == 1
    won = done & ((m[:, M_WINNER] == 1) == (root_role == 1))
    np.add.at(wins, (tt[won], jj[won]), 1)
    totals[1] = len(tt)
    totals[2] = int((~done).sum())
    if trace:
        st = np.concatenate(steps)
        st = st[np.lexsort((st["s"], st["copy"]))]
        assert moves.sum() == totals[0]
        return wins, totals, Trace(tt, jj, kk, moves, np.where(done, m[:, M_WINNER].astype(np.int64), -1), st, T)
    return wins, totals


def first_max_ids(wins, n, off, ids):
    """int32 [T]: the canonical id at the first maximum of wins[t][0 .. n[t]), -1 where the list is empty (ddz_playout_choose)"""
    out = np.full(len(n), -1, np.int32)
    for t in np.flatnonzero(n > 0):
        out[t] = ids[off[t] + int(np.argmax(wins[t, :n[t]]))]
    return out
