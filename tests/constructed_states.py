"""Constructed table states that put EVERY action id in front of the stepping kernels -- random play from a fresh deal
reaches about a fifth of the action space and none of the actions longer than 15 cards.  numpy only: no
GPU, no oracle, nothing of the reference; the action table (rows int8 [NA,15], info uint8 [NA,4] = category, value, len,
cards, as oracle.action_table() / the fixture action_table.npz hold it) is handed in.  Imported by
tests/test_constructed_states_cpu.py (which holds the builder and the CPU oracle to each other) and by
tests/test_gpu_constructed_states.py (which holds every stepping kernel to the oracle on these states).

States are packed uint8 [T][11][16] in the layout of include/ddz_env.h.  Every state built here is consistent
(check_consistent): per rank the three hands plus `taken` are the deck, `taken` is the sum of the histories, byte 15 of a
hand is its card count, a recent row carries its category byte, the meta row is as ddz_reset leaves it apart from role, ply
and episode (and what a step writes: done / winner / r).

Families (one table per action id):
  lead0       the lord at ply 0 holds the action among its 20 cards; where the deck allows the next player (down) holds a
              combination of the same category and length that beats it
  lead_exact  role r leads mid-game (ply >= 3, every recent row empty) and holds exactly the action: playing it wins
  step        the step rule of envi.py:38-43 in numpy: follow1 = step(lead0, ids), the next player faces the action
  skip_turn   follow2: the next player's turn skipped by hand -- the actor sees recent[role - 1] empty and recent[role + 1]
              = the action (what an import must read as one pass)
  edges       episode 0xFFFFFFF0, ply 250, a frozen and a never-dealt table among active ones
force_episode searches, per table, the smallest episode for which the engine RNG's draw of STEP_RANDOM selects a wanted
list index: so the kernels that take no selection (the rollouts) play the wanted id too."""
import numpy as np

ROW = 16
NFIELDS = 11
F_HAND0, F_HIST0, F_RECENT0, F_TAKEN, F_META = 0, 3, 6, 9, 10
M_ROLE, M_DONE, M_WINNER, M_REWARD, M_PLY, M_DEALT, M_EPISODE = 0, 1, 2, 3, 4, 6, 8
DECK = np.array([4] * 13 + [1, 1], np.int64)
DEALT = (17, 20, 17)                         # cards of role 0 up / 1 lord / 2 down (envi.py:23)
CARD_RANK = np.concatenate([np.repeat(np.arange(13), 4), [13, 14]])      # the 54 cards
CARD_SLOT = np.concatenate([np.tile(np.arange(4), 13), [0, 0]])          # position of a card within its rank
EDGE_EPISODE = 0xFFFFFFF0
EDGE_PLY = 250
MAX_TRIALS = 65536
EDGE_FROZEN, EDGE_UNDEALT = 7, 20            # where edges() puts the finished and the never-dealt table (of 32)


class Table:
    """the action table: rows int64 [NA,15], row16 uint8 [NA,16] (byte 15 = category), cat / value / length / cards [NA]"""

    def __init__(self, rows, info):
        rows = np.asarray(rows)[:, :15].astype(np.int64)
        info = np.asarray(info).astype(np.int64)
        self.rows = rows
        self.cat, self.value, self.length, self.cards = info[:, 0], info[:, 1], info[:, 2], info[:, 3]
        assert np.array_equal(rows.sum(1), self.cards) and not rows[0].any()
        self.n = rows.shape[0]
        self.row16 = np.zeros((self.n, ROW), np.uint8)
        self.row16[:, :15] = rows
        self.row16[:, 15] = self.cat
        self.key = pack_key(rows)
        self.order = np.argsort(self.key, kind="stable")
        assert np.all(np.diff(self.key[self.order]) > 0), "two action rows with the same counts"

    def lookup(self, counts):
        """action id of every count row of counts [...,15], -1 where it is no row of the table"""
        k = pack_key(counts)
        pos = np.minimum(np.searchsorted(self.key[self.order], k), self.n - 1)
        hit = self.key[self.order][pos] == k
        return np.where(hit, self.order[pos], -1)


def pack_key(counts):
    c = np.asarray(counts)[..., :15].astype(np.uint64)
    return (c << (np.arange(15, dtype=np.uint64) * np.uint64(4))).sum(-1, dtype=np.uint64)


# ---- engine RNG ------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (Salmon et al., SC'11) on arrays: counter words c0..c3 and key words k0, k1 broadcast against each
    other; returns the four output words as uint64 arrays of 32-bit values."""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3, k0, k1 = (np.asarray(x).astype(np.uint64) & M for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


def random_index(gid, episode, ply, n, seed):
    """the list index STEP_RANDOM takes on a list of n rows: (philox(gid lo, gid hi, episode, 2 << 16 | ply).x * n) >> 32"""
    gid = np.asarray(gid).astype(np.uint64)
    seed = int(seed)
    x = philox4x32_10(gid, gid >> np.uint64(32), episode, np.uint64(2 << 16) | np.asarray(ply).astype(np.uint64),
                      seed & 0xFFFFFFFF, seed >> 32)[0]
    return ((x * np.asarray(n).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def force_episode(states, index, n, seed, gid_base, max_trials=MAX_TRIALS):
    """Per table: the smallest episode < max_trials whose STEP_RANDOM draw selects list index `index` of a list of `n` rows
    (the table's ply and global id keyed in).  Returns (states with that episode in the meta row, trials int64 [T] = episodes
    tried, -1 where none of max_trials did: the caller asserts there is none)."""
    states = states.copy()
    T = states.shape[0]
    index, n = np.asarray(index).astype(np.int64), np.asarray(n).astype(np.int64)
    assert index.shape == (T,) and n.shape == (T,) and np.all((index >= 0) & (index < n))
    gid = np.uint64(gid_base) + np.arange(T, dtype=np.uint64)
    ply = meta_ply(states)
    ep = np.full(T, -1, np.int64)
    start, block = 0, 32
    while start < max_trials and (ep < 0).any():
        u = np.flatnonzero(ep < 0)
        block = min(block, max_trials - start)
        e = start + np.arange(block, dtype=np.int64)[None, :]
        got = random_index(gid[u, None], e, ply[u, None], n[u, None], seed)
        hit = got == index[u, None]
        has = hit.any(1)
        ep[u[has]] = start + hit.argmax(1)[has]
        start += block
        block = min(2 * block, 4096)
    ok = ep >= 0
    set_episode(states, np.where(ok, ep, 0))
    return states, np.where(ok, ep + 1, -1)


# ---- state rows ------------------------------------------------------------------------------------------------------------
def meta_ply(states):
    m = states[:, F_META]
    return m[:, M_PLY].astype(np.int64) | (m[:, M_PLY + 1].astype(np.int64) << 8)


def meta_episode(states):
    return np.ascontiguousarray(states[:, F_META, M_EPISODE:M_EPISODE + 4]).view("<u4")[:, 0].astype(np.int64)


def set_episode(states, episode):
    e = np.asarray(episode).astype(np.int64)
    for b in range(4):
        states[:, F_META, M_EPISODE + b] = (e >> (8 * b)) & 0xFF


def set_ply(states, ply):
    p = np.asarray(ply).astype(np.int64)
    states[:, F_META, M_PLY] = p & 0xFF
    states[:, F_META, M_PLY + 1] = (p >> 8) & 0xFF


def pack_state(hands, hist, role, ply, episode=0):
    """hands / hist int [T,3,15] -> running tables, every recent row empty, meta as ddz_reset leaves it apart from role,
    ply and episode"""
    T = hands.shape[0]
    s = np.zeros((T, NFIELDS, ROW), np.uint8)
    s[:, F_HAND0:F_HAND0 + 3, :15] = hands
    s[:, F_HAND0:F_HAND0 + 3, 15] = hands.sum(2)
    s[:, F_HIST0:F_HIST0 + 3, :15] = hist
    s[:, F_TAKEN, :15] = hist.sum(1)
    s[:, F_META, M_ROLE] = role
    s[:, F_META, M_WINNER] = 0xFF
    s[:, F_META, M_DEALT] = 1
    set_ply(s, np.broadcast_to(ply, (T,)))
    set_episode(s, np.broadcast_to(episode, (T,)))
    return s


def check_consistent(states, table):
    """assert every property the module's docstring promises, table by table (never-dealt tables: all zero)"""
    s = states.astype(np.int64)
    m = s[:, F_META]
    dealt = m[:, M_DEALT] == 1
    assert not s[~dealt].any(), "a never-dealt table is all zero"
    s, m, raw = s[dealt], m[dealt], states[dealt]
    hands, hist, recent, taken = s[:, 0:3, :15], s[:, 3:6, :15], s[:, 6:9], s[:, F_TAKEN, :15]
    assert np.array_equal(hands.sum(1) + taken, np.broadcast_to(DECK, taken.shape)), "hands + taken != the deck"
    assert np.array_equal(hist.sum(1), taken), "taken != sum of the histories"
    assert np.array_equal(s[:, 0:3, 15], hands.sum(2)), "byte 15 of a hand != its card count"
    assert not s[:, 3:6, 15].any() and not s[:, F_TAKEN, 15].any()
    rid = table.lookup(recent[..., :15])
    assert (rid >= 0).all(), "a recent row is no action"
    assert np.array_equal(recent[..., 15], table.cat[rid]), "a recent row's category byte"
    assert np.all((hist - recent[..., :15]) >= 0), "a recent row is not part of its role's history"
    done = m[:, M_DONE]
    assert np.all(m[:, M_ROLE] < 3) and np.all(done <= 1)
    left = s[:, 0:3, 15]
    assert np.array_equal(done == 1, (left == 0).any(1)), "done <=> an empty hand"
    winner = np.where(done == 1, (left == 0).argmax(1), 0xFF)
    assert np.array_equal(m[:, M_WINNER], winner)
    r = raw[:, F_META, M_REWARD].view(np.int8)
    assert np.all(r[done == 0] == 0) and np.array_equal(r[done == 1], np.where(winner[done == 1] == 1, -1, 1))
    assert not m[:, [7, 12, 13, 14, 15]].any()


# ---- dealing ---------------------------------------------------------------------------------------------------------------
def draw_cards(rng, avail, k):
    """a uniformly random k[t]-card subset of the multiset avail [T,15] per table -> counts int64 [T,15]"""
    avail = np.asarray(avail).astype(np.int64)
    k = np.broadcast_to(np.asarray(k).astype(np.int64), avail.shape[:1])
    assert np.all(avail >= 0) and np.all((k >= 0) & (k <= avail.sum(1)))
    have = CARD_SLOT[None, :] < avail[:, CARD_RANK]                    # [T,54]: the cards of the multiset
    keys = np.where(have, rng.random(have.shape), 2.0)
    rank = np.argsort(np.argsort(keys, axis=1, kind="stable"), axis=1, kind="stable")
    take = have & (rank < k[:, None])
    out = np.zeros(avail.shape, np.int64)
    for r in range(15):
        out[:, r] = take[:, CARD_RANK == r].sum(1)
    assert np.array_equal(out.sum(1), k)
    return out


def find_answers(table, ids, rng, max_cards=17, beats=None):
    """per action id: the id of a combination of the same category and length and a higher value (CardGroup.bigger_than's
    same-type rule, card.py:321-325) of at most max_cards cards that the deck holds TOGETHER with the action, chosen at
    random among those; -1 where the deck has none.  beats(a, b) (oracle.beats), if given, confirms every answer."""
    ids = np.asarray(ids).astype(np.int64)
    ans = np.full(len(ids), -1, np.int64)
    group = table.cat * 64 + table.length
    for g in np.unique(group[ids]):
        mine = np.flatnonzero(group[ids] == g)
        cand = np.flatnonzero((group == g) & (table.cards <= max_cards) & (np.arange(table.n) > 0))
        cand = cand[rng.permutation(len(cand))]
        for lo in range(0, len(mine) if len(cand) else 0, 128):
            a = ids[mine[lo:lo + 128]]
            fits = np.all(table.rows[a][:, None, :] + table.rows[cand][None, :, :] <= DECK, axis=2)
            fits &= table.value[cand][None, :] > table.value[a][:, None]
            has = fits.any(1)
            ans[mine[lo:lo + 128][has]] = cand[fits.argmax(1)[has]]
    if beats is not None:
        for a, b in zip(ids[ans >= 0], ans[ans >= 0]):
            assert beats(int(b), int(a)) and not beats(int(a), int(b))
    return ans


def lead0(table, ids, rng, beats=None):
    """LEAD0: one table per id at ply 0 -- the lord holds the action, filled to 20 cards; the next player (down) holds a
    same-category answer where find_answers has one; everything else dealt at random, 17 / 20 / 17.
    Returns (states, answers int64 [T]: the planted id or -1)."""
    ids = np.asarray(ids).astype(np.int64)
    assert np.all(table.cards[ids] <= DEALT[1])
    ans = find_answers(table, ids, rng, DEALT[2], beats)
    a = table.rows[ids]
    b = np.where(ans[:, None] >= 0, table.rows[np.maximum(ans, 0)], 0)
    avail = DECK - a - b
    fill = draw_cards(rng, avail, DEALT[1] - a.sum(1))
    avail = avail - fill
    down = draw_cards(rng, avail, DEALT[2] - b.sum(1))
    hands = np.stack([avail - down, a + fill, b + down], 1)
    return pack_state(hands, np.zeros_like(hands), role=1, ply=0), ans


def lead_exact(table, role, rng, ids=None):
    """LEAD-EXACT for role `role`: every id the role can hold (a farmer 17 cards, the lord 20), one table each.  The actor
    holds exactly the action and leads (every recent row empty) at a ply >= 3 at which it is this role's turn; the others
    hold 1 .. their dealt count cards, the rest of the deck lies in `taken`, split over the three histories by what each
    role has played (dealt - left).  Returns (ids, states)."""
    if ids is None:
        ids = np.flatnonzero(table.cards <= DEALT[role])
        ids = ids[ids > 0]
    ids = np.asarray(ids).astype(np.int64)
    T = len(ids)
    a = table.rows[ids]
    others = [(role + 1) % 3, (role + 2) % 3]
    hands = np.zeros((T, 3, 15), np.int64)
    hands[:, role] = a
    avail = DECK - a
    for o in others:
        hands[:, o] = draw_cards(rng, avail, rng.integers(1, DEALT[o] + 1, T))
        avail = avail - hands[:, o]
    hist = np.zeros((T, 3, 15), np.int64)
    for o in (role, others[0]):
        hist[:, o] = draw_cards(rng, avail, DEALT[o] - hands[:, o].sum(1))
        avail = avail - hist[:, o]
    hist[:, others[1]] = avail
    assert np.array_equal(avail.sum(1), DEALT[others[1]] - hands[:, others[1]].sum(1))
    # the lord moves at plies 0, 3, 6 ..., down at 1, 4, ..., up at 2, 5, ... (game.py:173-181): 3 .. 17, this role's turn
    ply = 3 + (role + 2) % 3 + 3 * (np.arange(T) % 5)
    return ids, pack_state(hands, hist, role=role, ply=ply)


# ---- the step rule (envi.py:38-43) -----------------------------------------------------------------------------------------
def step(states, table, ids):
    """Apply action ids[t] (legal by construction; the caller checks that against the oracle's lists) for the table's actor:
    hand - action, cards left - its size, history and taken + action, recent = the action with its category byte, then the
    next role, ply + 1, r (-1 the lord won, +1 a farmer), done / winner.  Finished and never-dealt tables stay as they are.
    No re-deal: what ddz_step does with auto_reset = 0."""
    s = states.copy()
    ids = np.asarray(ids).astype(np.int64)
    t = np.flatnonzero((s[:, F_META, M_DONE] == 0) & (s[:, F_META, M_DEALT] == 1))
    role = s[t, F_META, M_ROLE].astype(np.int64)
    a = table.rows[ids[t]].astype(np.uint8)
    assert np.all(s[t, F_HAND0 + role, :15] >= a), "the actor does not hold the action"
    s[t, F_HAND0 + role, :15] -= a
    s[t, F_HAND0 + role, 15] -= table.cards[ids[t]].astype(np.uint8)
    s[t, F_HIST0 + role, :15] += a
    s[t, F_TAKEN, :15] += a
    s[t, F_RECENT0 + role] = table.row16[ids[t]]
    won = s[t, F_HAND0 + role, 15] == 0
    s[t, F_META, M_ROLE] = (role + 1) % 3
    set_ply_rows = meta_ply(s[t]) + 1
    s[t, F_META, M_PLY] = set_ply_rows & 0xFF
    s[t, F_META, M_PLY + 1] = set_ply_rows >> 8
    s[t, F_META, M_REWARD] = np.where(won, np.where(role == 1, -1, 1), 0).astype(np.int8).view(np.uint8)
    s[t, F_META, M_DONE] = won
    s[t, F_META, M_WINNER] = np.where(won, role, 0xFF)
    return s


def skip_turn(states):
    """FOLLOW2 from FOLLOW1: the actor's turn passes by hand -- next role, ply + 1, its recent row zero.  What was
    recent[role - 1] = the action is now recent[role + 1], and recent[role - 1] is empty."""
    s = states.copy()
    assert not s[:, F_META, M_DONE].any() and s[:, F_META, M_DEALT].all()
    role = s[:, F_META, M_ROLE].astype(np.int64)
    s[np.arange(len(s)), F_RECENT0 + role] = 0
    s[:, F_META, M_ROLE] = (role + 1) % 3
    s[:, F_META, M_REWARD] = 0
    set_ply(s, meta_ply(s) + 1)
    return s


def running(states):
    return (states[:, F_META, M_DONE] == 0) & (states[:, F_META, M_DEALT] == 1)


def to_beat(states, table):
    """the action id the actor has to beat (envi.py:103-109: the previous player's handout, else the one before; 0 = lead)"""
    role = states[:, F_META, M_ROLE].astype(np.int64)
    t = np.arange(len(states))
    b1 = table.lookup(states[t, F_RECENT0 + (role + 2) % 3, :15])
    b2 = table.lookup(states[t, F_RECENT0 + (role + 1) % 3, :15])
    return np.where(b1 > 0, b1, np.maximum(b2, 0))


def edges(table, rng):
    """A handful of tables at the limits of the counters, a frozen and a never-dealt table among them:
      3n tables  lead_exact of role 0, 1, 2 (n ids each: the longest the role can hold, a rocket and a quad among them)
                 at ply 251 / 252 / 250 -- the packed record has 8 bits for it --, this role's turn
      2n tables  follow1 and follow2 (a 6-card action to beat) at ply 250 / 251
      all of these at episode 0xFFFFFFF0; in between, at EDGE_FROZEN, a table a 20-card lead has finished and, at
      EDGE_UNDEALT, one never dealt (all zero)."""
    n = 6
    parts = []
    for role in range(3):
        ok = np.flatnonzero(table.cards <= DEALT[role])[1:]
        ids = np.concatenate([ok[np.argsort(table.cards[ok], kind="stable")[-(n - 2):]],
                              np.flatnonzero(table.cat == 12)[:1], np.flatnonzero(table.cat == 4)[-1:]])
        _, s = lead_exact(table, role, rng, ids)
        set_ply(s, EDGE_PLY + (role + 1) % 3)       # 250 is down's turn, 251 up's, 252 the lord's
        parts.append(s)
    six = np.flatnonzero((table.cards == 6) & (table.value < 6))
    ids = six[rng.permutation(len(six))[:n]]
    s0, _ = lead0(table, ids, rng)
    f1 = step(s0, table, ids)
    f2 = skip_turn(f1)
    set_ply(f1, EDGE_PLY)
    set_ply(f2, EDGE_PLY + 1)
    parts += [f1, f2]
    s = np.concatenate(parts)
    set_episode(s, np.full(len(s), EDGE_EPISODE))
    won = np.flatnonzero(table.cards == DEALT[1])[:1]
    frozen = step(lead0(table, won, rng)[0], table, won)
    assert frozen[0, F_META, M_DONE] == 1
    # the two idle tables sit between running ones: inside a wave's chunk of tables, not at the batch's tail
    return np.concatenate([s[:EDGE_FROZEN], frozen, s[EDGE_FROZEN:EDGE_UNDEALT - 1], np.zeros((1, NFIELDS, ROW), np.uint8),
                           s[EDGE_UNDEALT - 1:]])


# ---- the families with their reference lists (the oracle module is handed in: this file imports numpy alone) ---------------
SEED = 9
GID_BASE = 2 ** 33 + 1000        # table_id_base above 2^32: the high word of the RNG counter is in play


class Family:
    """states uint8 [T,11,16]; off / rows / ids: the oracle's CSR lists of these states (shared by the tests: never written);
    n = list sizes; index / want: the list index and action id to play per table (-1: none, a frozen table);
    beat: the action id the actor faces (0 = lead); trials: episodes force_episode tried (forced families)"""

    def __init__(self, name, states, lists, index, beat, trials=None):
        self.name, self.states, self.T = name, states, len(states)
        self.off, self.rows, self.ids = lists
        self.n = np.diff(self.off).astype(np.int64)
        self.index = np.asarray(index).astype(np.int64)
        pick = self.off[:-1] + np.maximum(self.index, 0)
        self.want = np.where(self.index >= 0, self.ids[np.minimum(pick, len(self.ids) - 1)], -1).astype(np.int64)
        self.beat, self.trials = beat, trials


def oracle_env(oracle, states, seed=SEED, gid_base=GID_BASE):
    env = oracle.OracleEnv(len(states), seed=seed, gid_base=gid_base)
    env.state[:] = states.reshape(-1)
    return env


def oracle_lists(oracle, states):
    off, rows, ids = oracle_env(oracle, states).legal()
    return off.copy(), rows.copy(), ids.copy()


def wanted_index(off, list_ids, want):
    """the position of want[t] in table t's CSR list, -1 where the list does not hold it"""
    T = len(off) - 1
    n = np.diff(off)
    seg = np.repeat(np.arange(T), n)
    hit = np.flatnonzero(list_ids == np.asarray(want)[seg])
    idx = np.full(T, -1, np.int64)
    idx[seg[hit]] = hit - off[:-1][seg[hit]]
    return idx


def _forced(oracle, name, states, ids, beat):
    """the family with the episode forced.  Whether every id is in its table's list (legal) and every search resolved
    (trials > 0) is recorded, not asserted: tests/test_constructed_states_cpu.py asserts both by name."""
    lists = oracle_lists(oracle, states)
    idx = wanted_index(lists[0], lists[2], ids)
    states, trials = force_episode(states, np.maximum(idx, 0), np.maximum(np.diff(lists[0]), 1), SEED, GID_BASE)
    f = Family(name, states, lists, idx, beat, trials)
    f.legal = idx >= 0
    return f


def _spread(n):
    """a list index per table that depends on nothing but the table's number: (7919 t) mod n, -1 for an empty list"""
    return np.where(n > 0, (7919 * np.arange(len(n))) % np.maximum(n, 1), -1)


def families(oracle, table, first_id=1):
    """lead0 (ids first_id .. NA - 1), follow1 / follow2 behind it, and for first_id = 1 lead_exact (the three roles, one
    batch) and the edges.  The rng streams are fixed: the same states in every process."""
    ids = np.arange(first_id, table.n)
    rng = np.random.default_rng(0)
    s0, ans = lead0(table, ids, rng, oracle.beats)
    out = {"lead0": _forced(oracle, "lead0", s0, ids, np.zeros(len(ids), np.int64))}
    post = step(out["lead0"].states, table, ids)
    run = running(post)
    f1 = post[run]
    lists = oracle_lists(oracle, f1)
    planted = wanted_index(lists[0], lists[2], ans[run])
    assert np.array_equal(planted >= 0, ans[run] >= 0), "a planted answer is not legal"
    out["follow1"] = Family("follow1", f1, lists, np.where(planted >= 0, planted, _spread(np.diff(lists[0]))), ids[run])
    f2 = skip_turn(f1)
    lists = oracle_lists(oracle, f2)
    out["follow2"] = Family("follow2", f2, lists, _spread(np.diff(lists[0])), ids[run])
    if first_id == 1:
        parts = [lead_exact(table, role, np.random.default_rng(10 + role)) for role in range(3)]
        xs = np.concatenate([p[1] for p in parts])
        xi = np.concatenate([p[0] for p in parts])
        out["exact"] = _forced(oracle, "exact", xs, xi, np.zeros(len(xi), np.int64))
        e = edges(table, np.random.default_rng(20))
        lists = oracle_lists(oracle, e)
        out["edges"] = Family("edges", e, lists, _spread(np.diff(lists[0])), to_beat(e, table))
    return out


# ---- what a path must reproduce, and the comparison ------------------------------------------------------------------------
def reference_run(oracle, states, mode=0, sel=None, auto_reset=True, iters=1, seed=SEED, gid_base=GID_BASE):
    """`iters` lock-step iterations of the ORACLE from `states` (sel applies to the first; later ones draw): per iteration
    a dict of the pre-step CSR lists (off / rows / ids), done / reward / illegal, the 32-byte records (traj) and the whole
    packed state after the step (state); plus the statistics the engine accumulates over the run."""
    env = oracle_env(oracle, states, seed, gid_base)
    out = []
    for it in range(iters):
        off, rows, ids = (x.copy() for x in env.legal())
        done, reward, illegal, traj = env.step(mode if it == 0 else 0, sel if it == 0 else None, auto_reset=auto_reset,
                                               want_traj=True)
        out.append({"off": off, "rows": rows, "ids": ids, "done": done, "reward": reward, "illegal": illegal,
                    "traj": traj, "state": env.state.copy()})
    return out, run_stats([o["traj"] for o in out])


def run_stats(trajs):
    """{plies, episodes, lord_wins, up_wins, down_wins} of a run from its records: a ply is an applied action (flags 0)"""
    tr = np.stack(trajs)
    played, won = tr[..., 19] == 0, tr[..., 17] == 1
    wins = [int((played & won & (tr[..., 16] == r)).sum()) for r in range(3)]
    return {"plies": int(played.sum()), "episodes": int((played & won).sum()), "lord_wins": wins[1], "up_wins": wins[0],
            "down_wins": wins[2]}


def differences(got, want):
    """the names of the entries of `want` that `got` does not hold byte for byte (same shape, same item size, same bytes;
    plain ints and dicts of ints by value).  Empty list = the path computed what the oracle computed."""
    bad = []
    for k, w in want.items():
        if k not in got:
            bad.append(k + ": missing")
        elif isinstance(w, dict):
            bad += [k + "." + j for j in w if got[k].get(j) != w[j]]
        elif np.isscalar(w):
            if got[k] != w:
                bad.append(k)
        else:
            g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(w)
            if g.shape != w.shape or g.dtype.itemsize != w.dtype.itemsize or (g.dtype.kind == "f") != (w.dtype.kind == "f"):
                bad.append(k + ": shape / type")
            elif not np.array_equal(g.view(np.uint8), w.view(np.uint8)):
                at = np.flatnonzero((g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1)).any(1)) if g.ndim else []
                bad.append("%s: %d rows differ, first %s" % (k, len(at), at[:5].tolist() if len(at) else "?"))
    return bad
