"""Playout spec v2, hidden hands, restated on the CPU oracle: what ddz_playout_worlds and ddz_playout_hidden
must give, independent of the engine.  Written from the spec; numpy and the oracle module (handed in) only.

  unseen_r = deck_r - hand[role]_r - taken_r  (deck_r = 4 for the ranks 0..12, 1 for each joker)
  pool     = the cards c of Deal v2's numbering (rank c // 4 for c < 52, 52 = BJ, 53 = CJ) with (c & 3) < unseen_{c // 4},
             resp. unseen_13 = 1 / unseen_14 = 1
  n_next   = byte 15 of hand row (role + 1) % 3, n_prev = byte 15 of hand row (role + 2) % 3
  domain   = every unseen_r in [0, deck_r], n_next >= 1, n_prev >= 1, sum unseen = n_next + n_prev
  key_c    = philox4x32_10((gid_lo, gid_hi, k, 5 << 16 | c >> 2), (seed_lo ^ salt, seed_hi))[c & 3], gid = gid_base + t
  world k  = the pool ranked by (key, c): the n_next lowest cards to the next player, the others to the previous one
The 15 count bytes of the two opponents' hand rows are never read.  playouts_hidden() is the loop of
playout_reference.playouts (spec v1) on copies (t, j, k) whose opponent rows are world k."""
import numpy as np

import constructed_states as cs
import playout_reference as pr

ROW, NFIELDS = pr.ROW, pr.NFIELDS
F_HAND0, F_TAKEN, F_META = 0, 9, pr.F_META
DECK = np.array([4] * 13 + [1, 1], np.int64)
DOMAIN_WORLD = 5
CARD_RANK = np.array([c >> 2 for c in range(52)] + [13, 14])


def decode(states):
    """per table: (running, role, unseen int64 [15], n_next, n_prev, in the domain) -- read from the actor's hand row, the
    taken row, the meta row and byte 15 of the other two hand rows alone"""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    out = []
    for s in states:
        m = s[F_META]
        run = bool(m[pr.M_DEALT]) and not m[pr.M_DONE]
        role = int(m[pr.M_ROLE]) if m[pr.M_ROLE] <= 2 else 0
        unseen = DECK - s[F_HAND0 + role, :15].astype(np.int64) - s[F_TAKEN, :15].astype(np.int64)
        n_next, n_prev = int(s[F_HAND0 + (role + 1) % 3, 15]), int(s[F_HAND0 + (role + 2) % 3, 15])
        ok = bool((unseen >= 0).all() and (unseen <= DECK).all() and n_next >= 1 and n_prev >= 1
                  and unseen.sum() == n_next + n_prev)
        out.append((run, role, unseen, n_next, n_prev, ok))
    return out


def pool_cards(unseen):
    return [c for c in range(54) if (((c & 3) < unseen[c >> 2]) if c < 52 else unseen[c - 39] == 1)]


def world_cards(oracle, pool, n_next, gid, k, key, domain=DOMAIN_WORLD):
    """(cards of the next player, cards of the previous player) of world k: sorted card numbers"""
    draws = {}
    for g in sorted({c >> 2 for c in pool}):
        draws[g] = oracle.philox([gid & 0xFFFFFFFF, gid >> 32, k, (domain << 16) | g], key)
    ranked = sorted(pool, key=lambda c: (int(draws[c >> 2][c & 3]), c))
    return sorted(ranked[:n_next]), sorted(ranked[n_next:])


def rows_of(nxt, prv):
    """uint8 [2, 16]: the count row and byte 15 (the size) of the two hands"""
    out = np.zeros((2, ROW), np.uint8)
    for i, cards in enumerate((nxt, prv)):
        for c in cards:
            out[i, CARD_RANK[c]] += 1
        out[i, 15] = len(cards)
    return out


def worlds(oracle, states, n_worlds, seed=0, gid_base=0, salt=0, roles=0b111, out=None, domain=DOMAIN_WORLD):
    """-> (out uint8 [T, n_worlds, 2, 16], took_part bool [T], out_of_domain bool [T]): ddz_playout_worlds.  Tables that are
    idle, left out by `roles` or outside the domain keep what `out` held (zeros when none is handed in)."""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T, K = len(states), int(n_worlds)
    out = np.zeros((T, K, 2, ROW), np.uint8) if out is None else out
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    part, bad = np.zeros(T, bool), np.zeros(T, bool)
    for t, (run, role, unseen, n_next, n_prev, ok) in enumerate(decode(states)):
        if not run or not (roles >> role) & 1:
            continue
        if not ok:
            bad[t] = True
            continue
        part[t] = True
        pool = pool_cards(unseen)
        for k in range(K):
            out[t, k] = rows_of(*world_cards(oracle, pool, n_next, int(gid_base) + t, k, key, domain))
    return out, part, bad


def with_world(state, world):
    """a copy of one state [11, 16] whose opponents' hand rows are `world` [2, 16] (byte 15 = the row sum)"""
    s = np.array(state, np.uint8).reshape(NFIELDS, ROW).copy()
    role = int(s[F_META, pr.M_ROLE]) % 3
    s[F_HAND0 + (role + 1) % 3] = world[0]
    s[F_HAND0 + (role + 2) % 3] = world[1]
    for r in ((role + 1) % 3, (role + 2) % 3):
        s[F_HAND0 + r, 15] = s[F_HAND0 + r, :15].sum()
    return s


def playouts_hidden(oracle, states, n_playouts, seed=0, gid_base=0, salt=0, roles=0b111, stride=pr.STRIDE,
                    max_plies=pr.MAX_PLIES, the_worlds=None):
    """-> (wins int32 [T, stride], totals int64 [4], out_of_domain bool [T]) of playout spec v2: the loop of
    playout_reference.playouts on one copy per (t, j, k) whose opponents' rows are world k of table t.  the_worlds: use
    these (out, took_part, out_of_domain) instead of worlds() -- the perturbation controls hand in altered ones."""
    states = np.asarray(states, np.uint8).reshape(-1, NFIELDS, ROW)
    T, K = len(states), int(n_playouts)
    W, part, bad = the_worlds if the_worlds is not None else worlds(oracle, states, K, seed, gid_base, salt, roles)
    wins = np.zeros((T, stride), np.int32)
    totals = np.zeros(4, np.int64)
    n, _, _ = pr.root_lists(oracle, states, seed, gid_base)     # (the root's list: the actor's hand and the recent rows)
    n = np.where(part, n, 0)
    assert n.max(initial=0) <= stride
    tt = np.repeat(np.arange(T), n * K)
    if len(tt) == 0:
        return wins, totals, bad
    within = np.arange(len(tt)) - np.repeat(np.cumsum(n * K) - n * K, n * K)
    jj, kk = within // K, within % K
    copies = np.stack([with_world(states[t], W[t, k]) for t, k in zip(tt, kk)])
    env = oracle.OracleEnv(len(tt), seed=seed, gid_base=gid_base)
    env.state[:] = copies.reshape(-1)
    m = env.field(F_META)
    root_role = m[:, pr.M_ROLE].copy()
    env.legal()
    _, _, illegal, _ = env.step(pr.STEP_CHOICE, jj.astype(np.int32), auto_reset=False)
    assert not illegal.any()
    totals[0] += len(tt)
    gid = np.uint64(gid_base) + tt.astype(np.uint64)
    key = [(int(seed) ^ int(salt)) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    for it in range(max_plies - 1):
        off, _, _ = env.legal()
        A = np.diff(off).astype(np.int64)
        act = np.flatnonzero((m[:, pr.M_DONE] == 0) & (A > 0))
        if len(act) == 0:
            break
        ply = m[:, pr.M_PLY].astype(np.int64) | (m[:, pr.M_PLY + 1].astype(np.int64) << 8)
        sel = np.full(len(tt), -1, np.int32)
        # the draw of spec v1 (domain 4), for all copies at once: constructed_states.philox4x32_10 is the same function on
        # arrays (tests/test_playout_hidden_cpu.py holds this loop to playout_reference.playouts, which calls oracle.philox)
        draw = cs.philox4x32_10(gid[act], gid[act] >> np.uint64(32), (kk[act] << 9) | jj[act], (4 << 16) | ply[act], *key)[0]
        sel[act] = ((draw * A[act].astype(np.uint64)) >> np.uint64(32)).astype(np.int32)
        env.step(pr.STEP_CHOICE, sel, auto_reset=False)
        totals[0] += len(act)
    done = m[:, pr.M_DONE] == 1
    won = done & ((m[:, pr.M_WINNER] == 1) == (root_role == 1))
    np.add.at(wins, (tt[won], jj[won]), 1)
    totals[1] = len(tt)
    totals[2] = int((~done).sum())
    return wins, totals, bad
