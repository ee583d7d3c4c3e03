"""Playout spec v1 restated on the CPU oracle: what ddz_playout must count, independent of the engine.

Every root state is replicated once per (move index j, playout number k) into ONE OracleEnv; the root moves are applied with
STEP_CHOICE; then, until every copy is done, the loop is legal() -> index from oracle.philox -> step(STEP_CHOICE, no
auto-reset).  Nothing here touches the GPU library; numpy and the oracle module (handed in) only.
  draw  = philox4x32_10((gid_lo, gid_hi, k << 9 | j, 4 << 16 | ply), (seed_lo ^ salt, seed_hi)).x, gid = gid_base + t,
          ply = the u16 ply counter of the state being stepped
  index = (draw * A) >> 32 into the state's legal list of A moves; A = 0 on a running copy stops it (unfinished)
  wins[t][j] = the playouts of move j that ended with a winner on the root actor's side (the lord alone, or either farmer)
  totals = {moves applied (root moves included), playouts run, playouts stopped unfinished, 0}"""
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


def playouts(oracle, states, n_playouts, seed=0, gid_base=0, salt=0, stride=STRIDE, max_plies=MAX_PLIES):
    """-> (wins int32 [T, stride], totals int64 [4]) of playout spec v1 for `states` uint8 [T, 11, 16]"""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T, K = len(states), int(n_playouts)
    wins = np.zeros((T, stride), np.int32)
    totals = np.zeros(4, np.int64)
    n, _, _ = root_lists(oracle, states, seed, gid_base)
    assert n.max(initial=0) <= stride
    # one copy per (t, j, k); idle tables have n = 0 and get none
    tt = np.repeat(np.arange(T), n * K)
    if len(tt) == 0:
        return wins, totals
    within = np.arange(len(tt)) - np.repeat(np.cumsum(n * K) - n * K, n * K)
    jj, kk = within // K, within % K
    env = _env(oracle, states[tt], seed, gid_base)
    m = env.field(F_META)
    root_role = m[:, M_ROLE].copy()
    env.legal()
    _, _, illegal, _ = env.step(STEP_CHOICE, jj.astype(np.int32), auto_reset=False)
    assert not illegal.any()
    totals[0] += len(tt)
    gid = np.uint64(gid_base) + tt.astype(np.uint64)
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    stopped = np.zeros(len(tt), bool)
    for _ in range(max_plies - 1):
        off, _, _ = env.legal()
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
        env.step(STEP_CHOICE, sel, auto_reset=False)
        totals[0] += len(act)
    done = m[:, M_DONE] == 1
    won = done & ((m[:, M_WINNER] == 1) == (root_role == 1))
    np.add.at(wins, (tt[won], jj[won]), 1)
    totals[1] = len(tt)
    totals[2] = int((~done).sum())
    return wins, totals


def first_max_ids(wins, n, off, ids):
    """int32 [T]: the canonical id at the first maximum of wins[t][0 .. n[t]), -1 where the list is empty (ddz_playout_choose)"""
    out = np.full(len(n), -1, np.int32)
    for t in np.flatnonzero(n > 0):
        out[t] = ids[off[t] + int(np.argmax(wins[t, :n[t]]))]
    return out
