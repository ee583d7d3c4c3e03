"""Imported states, built key by key, for the shared-row finders (csrc/ddz_qnet.h sections 5, 5b, 6, 7: ddz_q_shared_rows,
ddz_q_shared_rows_hashed, ddz_q_roles_rows, ddz_q_shared_need / ddz_q_roles_need).  States that play reaches from a fresh deal
never occupy the last 21 chunks of a rank of the direct-addressed table, never fill a hashed region beyond a few per cent and
never wrap a probe chain; these do.  numpy only: no GPU, no oracle, nothing of the reference.  Imported by
tests/test_shared_row_states_cpu.py (which holds the builder to its own description, the keys to face_columns and face_columns
to the CPU oracle) and by tests/test_gpu_shared_row_finders.py (which holds the finders to the expectations stated here).

A state is uint8 [T][11][16] in the layout of include/ddz_env.h: fields 0..2 the hands (byte 15 = cards left), 3..5 the
histories, 6..8 the recent handouts, 9 taken, 10 meta (byte 0 = role).  The states are NOT consistent games: the finders,
ddz_observe and the first-layer kernels read bytes only, and no legal-move list is ever built from them.  What a face does not
read (the other hands' rank bytes, the actor's own recent row and card count) is filled with seeded noise: it must not matter.

The keys are restated from the documentation (ddz_env.h, ddz_qnet.h sections 5, 5b, 7):
  direct_key   rank * 275,625 + (((hand * 5 + taken) * 5 + b1) * 5 + b2) * 441 + ncode; fields saturated at 4, the two opponents'
               card counts saturated at 20 then reduced by their gcd, ncode = n1 * 21 + n2, or 0 where hand + taken >= total
  hash_key     the stored word key + 1; key = rank (4 bits) | hand, taken, h(role - 1), h(role), h(role + 1)[, b1, b2] saturated at
               4 (3 bits each) | the direct key's ncode (9 bits): 28 bits for variant 1, 34 for variant 2
  Both keys have ONE documented domain: card counts (byte 15 of a hand row) <= 20; count bytes above 4 and role bytes above 2
  are inside it.  Beyond it (25, 5) reads as (20, 5): two columns, one row.
  home         murmur3's 64-bit finaliser of the stored word, masked to the region
face_columns is the independent ground truth for "equal key <=> may share a row": the column of every (table, rank) from the
bytes, as ddz_observe is documented (thermometer count > j; prob n / (n1 + n2) in fp32 where known <= j < total; a role byte
above 2 reads as role 0).

Families (family(name, variant, T)):
  every_field   T 1250: all 625 (hand, taken, b1, b2) combinations on every rank (rotated per rank), every value 0..4 of the
                history fields on every rank, all 441 raw (n1, n2) pairs in 0..20 (every canonical pair and its multiples), the
                three roles
  chunk_edges   direct; T <= 4096: per rank the valid codes nearest to both sides of every chunk boundary c * 2048, code 0 and the
                largest code 275,184 on every rank (so on adjacent ranks), both valid codes of the partial last chunk, and every
                valid code of chunks 0..2 (258 of 441 slots per combination: all four waves of the assign scan carry)
  full_load     hashed; T 1024 (region 2048: load exactly 1/2) and 1025 (region 4096): the T keys of a rank distinct and all homed
                in the last W slots of the region, so the cluster wraps to slot 0 and probes run for hundreds of slots
  one_home      hashed; T 1024: 64 distinct keys per rank homed in one window, each held by 16 tables -- "block": the 16 copies in
                16 consecutive tables (one 256-thread block of the mark kernel, four copies per wave: a wave holds four tables),
                "spread": in 16 different blocks.  The window is ONE slot for variant 2; variant 1 has 1250 field combinations
                per (rank, pair) for 2048 home slots, so one slot cannot hold 64 keys whose tables share their (n1, n2): its
                window is ONE_HOME_WINDOW[1] slots
  tiny          T 1 and 37 (a ragged last block), in-domain random fields
  domain_edges  T 64: one base table repeated with count bytes 4, 5, 7, 255 in every key field, role bytes 3 and 255, and left
                bytes 0, 20, 21, 25, 255 on either opponent -- (25, 5) beside (20, 5) among them
  roles         T 1024: variants 1 / 2 the full_load states (every slot's regions get a wrapped cluster); variant 3 every_field's
                first 1024 tables with code 0 and the largest code on every rank in every role (the last key of slot s / rank 14
                and the first key of slot s + 1 / rank 0 are both occupied)
"""
import functools

import numpy as np

ROW, NFIELDS = 16, 11
F_HAND0, F_HIST0, F_RECENT0, F_TAKEN, F_META = 0, 3, 6, 9, 10
PLANES = {1: 7, 2: 9, 3: 6}
QSH_COLS = 625 * 441
QSH_KEYS = 15 * QSH_COLS
QSH_CHUNK = 2048
QSH_CPR = (QSH_COLS + QSH_CHUNK - 1) // QSH_CHUNK                # 135
LARGEST_CODE = 624 * 441                                        # 275,184: (4, 4, 4, 4), no prob slot left
TOTAL = np.array([4] * 13 + [1, 1], np.int64)
KEY_FIELDS = {1: ("hand", "taken", "hm1", "h0", "hp1"), 2: ("hand", "taken", "hm1", "h0", "hp1", "b1", "b2"),
              3: ("hand", "taken", "b1", "b2")}
FIELD_NAMES = ("hand", "taken", "hm1", "h0", "hp1", "b1", "b2")
ROLE_MAPS = ([0, 1, 2], [0, 0, -1], [-1, 0, -1], [1, -1, 0])
# full_load: window of home slots at the end of the region (ranks 0..12, the two joker ranks); the caps of the family are
# 64 / 256 for variant 1 and 64 / 16 for variant 2
FULL_LOAD_WINDOW = {1: (64, 256), 2: (4, 8)}
ONE_HOME_WINDOW = {1: (8, 16), 2: (1, 1)}
ONE_HOME_FIRST = 1000                                           # first home slot of the one_home window


def hash_region(T):
    """slots per rank region of the hashed table: max(2048, the power of two >= 2 T)"""
    r = QSH_CHUNK
    while r < 2 * T:
        r <<= 1
    return r


# ---- packing ---------------------------------------------------------------------------------------------------------------
def state_from_fields(role, n1, n2, hand, taken, hm1=0, h0=0, hp1=0, b1=0, b2=0, noise_seed=1):
    """role, n1, n2 [T] and the seven per-(table, rank) counts [T,15] (bytes 0..255; scalars broadcast) -> uint8 [T,11,16].
    role is the byte written; the fields are placed relative to the role the kernels read (a byte above 2 reads as 0):
    hand in the actor's hand row, n1 / n2 in byte 15 of the next / previous player's hand, hm1 / h0 / hp1 the histories of
    (role - 1, role, role + 1), b1 / b2 the recent handouts of (role - 1, role + 1)."""
    role = np.asarray(role).astype(np.int64)
    T = role.shape[0]
    f = {k: np.broadcast_to(np.asarray(v, np.int64), (T, 15)) for k, v in
         dict(hand=hand, taken=taken, hm1=hm1, h0=h0, hp1=hp1, b1=b1, b2=b2).items()}
    n1, n2 = np.broadcast_to(np.asarray(n1, np.int64), (T,)), np.broadcast_to(np.asarray(n2, np.int64), (T,))
    for v in list(f.values()) + [role, n1, n2]:
        assert v.min() >= 0 and v.max() <= 255
    rng = np.random.default_rng(noise_seed)
    st = np.zeros((T, NFIELDS, ROW), np.uint8)
    st[:, F_HAND0:F_HAND0 + 3] = rng.integers(0, 256, (T, 3, ROW))            # unread: overwritten where a face reads
    st[:, F_RECENT0:F_RECENT0 + 3] = rng.integers(0, 256, (T, 3, ROW))
    st[:, F_HIST0:F_HIST0 + 3, 15] = rng.integers(0, 256, (T, 3))
    st[:, F_TAKEN, 15] = rng.integers(0, 256, T)
    eff = np.where(role > 2, 0, role)
    rm1, rp1 = (eff + 2) % 3, (eff + 1) % 3
    ar = np.arange(T)
    st[ar, F_HAND0 + eff, :15] = f["hand"]
    st[:, F_TAKEN, :15] = f["taken"]
    st[ar, F_HIST0 + rm1, :15], st[ar, F_HIST0 + eff, :15], st[ar, F_HIST0 + rp1, :15] = f["hm1"], f["h0"], f["hp1"]
    st[ar, F_RECENT0 + rm1, :15], st[ar, F_RECENT0 + rp1, :15] = f["b1"], f["b2"]
    st[ar, F_HAND0 + rp1, 15], st[ar, F_HAND0 + rm1, 15] = n1, n2
    st[:, F_META, 0] = role
    return st


def fields_of_state(state):
    """the bytes the faces read, from a packed state: dict of int64 arrays (role = the byte; eff = the role it reads as)"""
    st = np.asarray(state).reshape(-1, NFIELDS, ROW)
    T = st.shape[0]
    role = st[:, F_META, 0].astype(np.int64)
    eff = np.where(role > 2, 0, role)
    rm1, rp1 = (eff + 2) % 3, (eff + 1) % 3
    ar = np.arange(T)
    i64 = lambda x: x.astype(np.int64)                                         # noqa: E731
    return {"role": role, "eff": eff, "n1": i64(st[ar, F_HAND0 + rp1, 15]), "n2": i64(st[ar, F_HAND0 + rm1, 15]),
            "hand": i64(st[ar, F_HAND0 + eff, :15]), "taken": i64(st[:, F_TAKEN, :15]),
            "hm1": i64(st[ar, F_HIST0 + rm1, :15]), "h0": i64(st[ar, F_HIST0 + eff, :15]), "hp1": i64(st[ar, F_HIST0 + rp1, :15]),
            "b1": i64(st[ar, F_RECENT0 + rm1, :15]), "b2": i64(st[ar, F_RECENT0 + rp1, :15])}


# ---- the keys ----------------------------------------------------------------------------------------------------------------
def _reduced(n1, n2):
    g = np.gcd(n1, n2)
    g = np.where(g < 1, 1, g)
    return n1 // g, n2 // g


def _saturated(f):
    """hand + taken >= total (no prob slot left), from the fields saturated at 4: the same truth value as on the raw bytes"""
    return np.minimum(f["hand"], 4) + np.minimum(f["taken"], 4) >= TOTAL[None, :]


def direct_key(state):
    """int64 [T,15]: the slot of (t, r) in the direct-addressed table of ddz_q_shared_rows"""
    f = fields_of_state(state)
    a, b = _reduced(np.minimum(f["n1"], 20), np.minimum(f["n2"], 20))
    ncode = np.where(_saturated(f), 0, (a * 21 + b)[:, None])
    combo = np.zeros_like(f["hand"])
    for k in KEY_FIELDS[3]:
        combo = combo * 5 + np.minimum(f[k], 4)
    return np.arange(15)[None, :] * QSH_COLS + combo * 441 + ncode


def hash_key(state, variant):
    """uint64 [T,15]: the word ddz_q_shared_rows_hashed stores for (t, r) (key + 1)"""
    f = fields_of_state(state)
    a, b = _reduced(np.minimum(f["n1"], 20), np.minimum(f["n2"], 20))
    ncode = np.where(_saturated(f), 0, (a * 21 + b)[:, None])
    key = np.broadcast_to(np.arange(15, dtype=np.int64)[None, :], f["hand"].shape).copy()
    for k in KEY_FIELDS[variant]:
        key = key << 3 | np.minimum(f[k], 4)
    return (key << 9 | ncode).astype(np.uint64) + np.uint64(1)


def hash_key_bits(variant):
    return 4 + 3 * len(KEY_FIELDS[variant]) + 9


def mix64(x):
    """murmur3's 64-bit finaliser on uint64 arrays"""
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def home_slot(words, R):
    return (mix64(words) & np.uint64(R - 1)).astype(np.int64)


def slot_of_tables(state, net_of_role):
    """int64 [T]: the network slot of every table under a role map (-1: a rule table); a role byte above 2 reads as role 0"""
    return np.asarray(net_of_role, np.int64)[fields_of_state(state)["eff"]]


def roles_direct_key(state, net_of_role):
    """the slot prefix of ddz_q_roles_rows, variant 3: slot * 4,134,375 + direct_key (-1 for a rule table); variants 1 / 2 keep
    hash_key and probe inside region slot * 15 + rank"""
    s = slot_of_tables(state, net_of_role)[:, None]
    return np.where(s < 0, -1, s * QSH_KEYS + direct_key(state))


def finder_key(state, variant):
    """the key of (t, r) WITHOUT its rank: what np.unique orders inside a rank's segment (variant 3) / the stored word (1, 2)"""
    return direct_key(state) if variant == 3 else hash_key(state, variant)


# ---- the faces -----------------------------------------------------------------------------------------------------------------
def face_columns(state, variant):
    """float32 [T,15,4 P]: the face column of every (table, rank), plane-major, from the bytes"""
    f = fields_of_state(state)
    T, P = f["hand"].shape[0], PLANES[variant]
    j = np.arange(4, dtype=np.int16)[None, None, :]
    out = np.empty((P, T, 15, 4), np.float32)
    for p, k in enumerate(KEY_FIELDS[variant]):
        out[p] = f[k].astype(np.int16)[:, :, None] > j                        # thermometer: slot j set iff count > j
    s = (f["n1"] + f["n2"]).astype(np.float32)
    known = (f["hand"] + f["taken"]).astype(np.int16)[:, :, None]
    open_ = (j >= known) & (j < TOTAL.astype(np.int16)[None, :, None])
    for p, n in ((P - 2, f["n1"]), (P - 1, f["n2"])):
        with np.errstate(divide="ignore", invalid="ignore"):
            fr = np.where(s > 0, n.astype(np.float32) / s, np.float32(0)).astype(np.float32)   # one fp32 division
        out[p] = np.where(open_, fr[:, None, None], np.float32(0))
    out = np.ascontiguousarray(out.transpose(1, 2, 0, 3))
    return out.reshape(T, 15, 4 * P)


def face(state, variant):
    """float32 [T,P,15,4]: ddz_observe's layout of face_columns"""
    c = face_columns(state, variant)
    return np.ascontiguousarray(c.reshape(c.shape[0], 15, PLANES[variant], 4).transpose(0, 2, 1, 3))


# ---- linear probing ----------------------------------------------------------------------------------------------------------
def occupied_slots(words, R):
    """the sorted slots a linear-probing table of R slots holds after the DISTINCT words were inserted at their homes, in any
    order: the slots depend on the multiset of homes alone (a slot is occupied iff a key homed at it or an insert passed over
    it), so carry the inserts that did not fit round the ring."""
    words = np.unique(np.asarray(words, np.uint64))
    assert words.size <= R
    c = np.bincount(home_slot(words, R), minlength=R)
    occ = np.zeros(R, bool)
    carry = 0
    for rnd in range(2):                    # the second round places what the first carried over the end
        for i in range(R):
            have = carry + (int(c[i]) if rnd == 0 else 0)
            if have and not occ[i]:
                occ[i] = True
                have -= 1
            carry = have
        if carry == 0:
            break
    assert carry == 0 and int(occ.sum()) == words.size
    return np.flatnonzero(occ)


# ---- what the finders must produce ---------------------------------------------------------------------------------------------
def seg_words(rows_per_rank, tile, capacity=None):
    """(q_reference.seg_table restated with an overflow form: this module is numpy only and must not import torch)
    int32 [40] in the finders' layout: [r] first row of rank r (a multiple of the tile), [15] rows in use, [16 + r] first
    tile, [31] tiles in use, [32] rows needed, [33] overflow (the segments end at the capacity then)"""
    seg = np.zeros(40, np.int32)
    row = 0
    for r, n in enumerate(rows_per_rank):
        seg[r], seg[16 + r] = row, row // tile
        row += (int(n) + tile - 1) // tile * tile
    over = capacity is not None and row > capacity
    if over:
        row = capacity // tile * tile
    seg[15], seg[31], seg[32], seg[33] = row, row // tile, int(sum(int(n) for n in rows_per_rank)), int(over)
    return seg


def check_finder(keys, rows, rep, seg, tile, all_keys, ordered, region=None):
    """one partition of a finder's output against the keys.  keys [n,15] of the partition's tables (any integer type), rows
    [n,16] partition-relative, rep / seg the partition's, all_keys [T,15] (what an instance number 16 t + r of rep is looked
    up in).  ordered: rows are numbered in key order (the direct table); else (hashed, region slots
    per rank) in slot order of a table whose occupied set is occupied_slots(keys of the rank).  Raises AssertionError."""
    keys, rows, rep, seg = np.asarray(keys), np.asarray(rows).astype(np.int64), np.asarray(rep).astype(np.int64), np.asarray(seg)
    n = keys.shape[0]
    assert rows.shape == (n, 16) and (rows[:, 15] == -1).all(), "column 15"
    uniq = [np.unique(keys[:, r]) for r in range(15)]
    want_seg = seg_words([u.size for u in uniq], tile)
    assert np.array_equal(seg[:34], want_seg[:34]), ("seg", seg[:34].tolist(), want_seg[:34].tolist())
    used = np.zeros(rep.shape[0], bool)
    flat_keys = np.asarray(all_keys).reshape(-1)
    for r in range(15):
        lo, u = int(want_seg[r]), uniq[r]
        col = rows[:, r]
        assert ((col >= lo) & (col < lo + u.size)).all(), f"rank {r}: a row outside its segment"
        rk = rep[lo: lo + u.size]
        assert (rk >= 0).all() and ((rk & 15) == r).all(), f"rank {r}: rep"
        row_key = flat_keys[(rk >> 4) * 15 + r]                               # the key every row stands for
        assert np.array_equal(row_key[col - lo], keys[:, r]), f"rank {r}: a table's row stands for another key"
        assert np.unique(row_key).size == u.size, f"rank {r}: two rows for one key"
        if ordered:
            assert np.array_equal(row_key, u), f"rank {r}: rows are not in key order"
        else:
            occ = occupied_slots(u, region)
            assert occ.size == u.size
            isocc = np.zeros(region, bool)
            isocc[occ] = True
            pre = np.concatenate([[0], np.cumsum(~isocc)])                    # empty slots before slot i
            home, slot = home_slot(row_key, region), occ                      # row i sits in the i-th occupied slot
            gaps = np.where(home <= slot, pre[slot + 1] - pre[home], (pre[region] - pre[home]) + pre[slot + 1])
            assert (gaps == 0).all(), f"rank {r}: a row whose slot is not reached from its key's home over occupied slots"
        used[lo: lo + u.size] = True
    assert (rep[~used] == -1).all(), "rep of a padding row / behind the segments"
    return want_seg


def expected_direct(state, tile, tables=None):
    """(rows [n,16], rep-free row keys, seg): the direct finder's exact output for the tables of a partition (all by default)"""
    keys = direct_key(state)
    if tables is not None:
        keys = keys[tables]
    uniq = [np.unique(keys[:, r]) for r in range(15)]
    seg = seg_words([u.size for u in uniq], tile)
    rows = np.full((keys.shape[0], 16), -1, np.int64)
    for r in range(15):
        rows[:, r] = seg[r] + np.searchsorted(uniq[r], keys[:, r])
    return rows, uniq, seg


def need_columns():
    """(rank, count) of the 54 row_index columns: 4 r + c - 1 for r < 13, 52 / 53 the jokers (count 1)"""
    col = np.arange(54)
    return np.where(col < 52, col >> 2, 13 + col - 52), np.where(col < 52, (col & 3) + 1, 1)


def expected_need(row_index, rows, sseg, tile, capacity=None):
    """ddz_q_shared_need stated in numpy: the D rows are the distinct (shared row s, count c) pairs some table needs
    (row_index[t][col] >= 0 and rows[t][rank of col] >= 0), in ascending 4 s + c - 1 order inside each rank's shared segment.
    -> (row_index2 [T,64], drep [n], row_cnt [n], dseg [40], n) with n = the rows written (dseg[15], or up to the capacity)."""
    row_index, rows, sseg = np.asarray(row_index), np.asarray(rows).astype(np.int64), np.asarray(sseg).astype(np.int64)
    T = rows.shape[0]
    rk, cnt = need_columns()
    s = rows[:, rk]                                                           # [T,54]
    need = (row_index[:, :54] >= 0) & (s >= 0)
    e = np.where(need, 4 * s + cnt[None, :] - 1, -1)
    ue = np.unique(e[need])
    rank_of = np.searchsorted(sseg[1:15], ue >> 2, side="right")             # rank of the segment that holds shared row s
    per_rank = np.bincount(rank_of, minlength=15)
    dseg = seg_words(per_rank, tile, capacity)
    first = np.concatenate([[0], np.cumsum(per_rank)[:-1]])
    drow = np.asarray(seg_words(per_rank, tile)[:15], np.int64)[rank_of] + np.arange(ue.size) - first[rank_of]   # unconstrained
    n = int(dseg[15])                                                         # (an overflow: the capacity; rows behind it are dropped)
    keep = drow < n
    ri2 = np.full((T, 64), -1, np.int64)
    if ue.size:
        d = np.where(keep, drow, -1)[np.minimum(np.searchsorted(ue, np.where(need, e, ue[0])), ue.size - 1)]
        ri2[:, :54] = np.where(need, d, -1)
    drep = np.full(n, -1, np.int64)
    row_cnt = np.zeros(n, np.int64)
    drep[drow[keep]] = ue[keep]
    row_cnt[drow[keep]] = (ue[keep] & 3) + 1
    return ri2, drep, row_cnt, dseg, n


def check_need(row_index, rows, sseg, tile, ri2, drep, row_cnt, dseg, capacity=None):
    """a partition's ddz_q_shared_need output against expected_need, exactly.  row_cnt is compared on the live D rows: the
    header leaves the count byte of a padding row inside a segment unspecified (the product of a padding row is never read)"""
    w_ri2, w_drep, w_cnt, w_dseg, n = expected_need(row_index, rows, sseg, tile, capacity)
    dseg, drep, row_cnt = np.asarray(dseg), np.asarray(drep).astype(np.int64), np.asarray(row_cnt).astype(np.int64)
    assert np.array_equal(dseg[:34], w_dseg[:34]), ("dseg", dseg[:34].tolist(), w_dseg[:34].tolist())
    assert np.array_equal(np.asarray(ri2).astype(np.int64), w_ri2), "row_index2"
    assert np.array_equal(drep[:n], w_drep), "drep"
    live = w_drep >= 0
    assert np.array_equal(row_cnt[:n][live], w_cnt[live]), "row_cnt"
    return n


# ---- families ----------------------------------------------------------------------------------------------------------------
def _digits(x, n):
    """x -> its n base-5 digits, most significant first"""
    return [(x // 5 ** (n - 1 - i)) % 5 for i in range(n)]


@functools.lru_cache(maxsize=None)
def canonical_pairs():
    """the gcd-reduced (n1, n2) of 0..20 x 0..20 in ncode order: int64 [258,2]"""
    a, b = np.meshgrid(np.arange(21), np.arange(21), indexing="ij")
    ra, rb = _reduced(a.reshape(-1), b.reshape(-1))
    return np.unique(np.stack([ra, rb], 1), axis=0)


@functools.lru_cache(maxsize=None)
def valid_codes(joker):
    """sorted column codes a state with fields in 0..4 and card counts in 0..20 can have on a rank < 13 / a joker rank"""
    total = 1 if joker else 4
    nc = canonical_pairs() @ np.array([21, 1])
    out = []
    for combo in range(625):
        hand, taken, _, _ = _digits(combo, 4)
        out.append(combo * 441 + (np.zeros(1, np.int64) if hand + taken >= total else nc))
    return np.unique(np.concatenate(out))


def _fields_of_code(code):
    """column code -> (hand, taken, b1, b2, n1, n2); n1 = n2 = -1: any pair (the code has no prob part)"""
    combo, nc = code // 441, code % 441
    hand, taken, b1, b2 = _digits(combo, 4)
    return hand, taken, b1, b2, nc // 21, nc % 21


def every_field(T=1250):
    t = np.arange(T)[:, None]
    r = np.arange(15)[None, :]
    hand, taken, b1, b2 = _digits((t + 97 * r) % 625, 4)
    hm1, h0, hp1 = (t + r) % 5, (t // 5 + 2 * r) % 5, (t // 25 + 3 * r) % 5
    tt = np.arange(T)
    pair = tt % 441
    return state_from_fields((tt + tt // 441) % 3, pair // 21, pair % 21, hand, taken, hm1, h0, hp1, b1, b2, noise_seed=2)


def boundary_codes(joker):
    """for every chunk boundary c * 2048 (c = 1..134) the valid code nearest below it and the one nearest at or above it"""
    v = valid_codes(joker)
    out = []
    for c in range(1, QSH_CPR):
        i = int(np.searchsorted(v, c * QSH_CHUNK))
        assert 0 < i < v.size
        out += [int(v[i - 1]), int(v[i])]
    return out


@functools.lru_cache(maxsize=None)
def chunk_edges():
    """the direct table's edges (read-only): every table holds one code per rank under ONE (n1, n2)"""
    tabs = []                                                        # [pair or None, [code or None] * 15]
    # every valid code of chunks 0..2: combinations 0..13 (hand = taken = 0) x every canonical pair, the same on all ranks
    for combo in range(14):
        for a, b in canonical_pairs():
            code = combo * 441 + int(a) * 21 + int(b)
            if code < 3 * QSH_CHUNK:
                tabs.append([(int(a), int(b)), [code] * 15])
    # the boundary codes, first fit into tables of their own (the tables above are full): a code with a prob part needs its
    # pair, one without (a saturated combination) fits under any
    dense = len(tabs)
    have = [{tb[1][r] for tb in tabs} for r in range(15)]
    for r in range(15):
        for code in boundary_codes(r >= 13):
            if code in have[r]:
                continue
            hand, taken, _, _, a, b = _fields_of_code(code)
            anyp = hand + taken >= TOTAL[r]
            for tb in tabs[dense:]:
                if tb[1][r] is None and (anyp or tb[0] == (a, b)):
                    tb[1][r] = code
                    break
            else:
                row = [None] * 15
                row[r] = code
                tabs.append([(5, 3) if anyp else (a, b), row])
            have[r].add(code)
    tabs.append([(7, 9), [LARGEST_CODE] * 15])                     # (code 0 is in chunk 0 above: (n1, n2) = (0, 0))
    T = len(tabs)
    assert T <= 4096
    f = np.zeros((6, T, 15), np.int64)
    n = np.zeros((2, T), np.int64)
    for t, (pair, codes) in enumerate(tabs):
        mult = 1 + t % max(1, 20 // max(pair[0], pair[1], 1))            # a multiple of the canonical pair, still <= 20
        n[:, t] = pair[0] * mult, pair[1] * mult
        for r in range(15):
            code = LARGEST_CODE if codes[r] is None else codes[r]    # the filler: the largest code, valid under any pair
            f[:4, t, r] = _fields_of_code(code)[:4]
    tt = np.arange(T)
    st = state_from_fields(tt % 3, n[0], n[1], f[0], f[1], 0, 0, 0, f[2], f[3], noise_seed=3)
    st.setflags(write=False)
    return st


def _combos(variant, joker, limit, rng):
    """field combinations [n, fields] whose key keeps its (n1, n2) part: hand + taken < total"""
    nf = len(KEY_FIELDS[variant])
    rest = 5 ** (nf - 2)
    ht = [(0, 0)] if joker else [(h, k) for h in range(5) for k in range(5) if h + k < 4]
    n_all = len(ht) * rest
    pick = np.arange(n_all) if n_all <= limit else np.sort(rng.choice(n_all, limit, replace=False))
    out = np.zeros((pick.size, nf), np.int64)
    out[:, :2] = np.asarray(ht)[pick // rest]
    out[:, 2:] = np.stack(_digits(pick % rest, nf - 2), 1)
    return out


def _words(variant, r, combos, a, b):
    key = np.full(combos.shape[0], r, np.int64)
    for i in range(combos.shape[1]):
        key = key << 3 | combos[:, i]
    return (key << 9 | (a * 21 + b)).astype(np.uint64) + np.uint64(1)


def _clustered(variant, R, groups, windows, first, seed, per_pair=8):
    """`groups` tables' worth of fields whose 15 keys home inside the rank's window [first, first + W) of a region of R slots:
    distinct keys per rank over the groups -- always for ranks 0..12, and for a joker rank while its window has an unused key
    under the table's pair (then an earlier key of that rank and pair is repeated).  The one (n1, n2) of a table is shared by
    its 15 ranks, so the search goes pair by pair (a fixed permutation of the canonical pairs of 0..20) and takes for every
    rank the combinations of that pair that home in the window.  -> (fields [groups,15,nf], pairs [groups,2], distinct [15])"""
    rng = np.random.default_rng(seed)
    nf = len(KEY_FIELDS[variant])
    combos = [_combos(variant, r >= 13, 4 * R, rng) for r in (0, 13)]
    pairs = canonical_pairs()
    pairs = pairs[(pairs[:, 0] + pairs[:, 1]) > 0]
    pairs = pairs[rng.permutation(pairs.shape[0])]
    fields = np.zeros((groups, 15, nf), np.int64)
    out_pairs = np.zeros((groups, 2), np.int64)
    distinct = np.zeros(15, np.int64)
    g = 0
    for a, b in pairs:
        if g == groups:
            break
        cand = []
        for r in range(15):
            cs = combos[r >= 13]
            w = windows[r >= 13]
            h = home_slot(_words(variant, r, cs, int(a), int(b)), R)
            cand.append(cs[(h >= first[r >= 13]) & (h < first[r >= 13] + w)])
        m = min(per_pair, groups - g, min(c.shape[0] for c in cand[:13]))
        if m == 0 or min(c.shape[0] for c in cand[13:]) == 0:
            continue
        for r in range(15):
            c = cand[r]
            idx = np.arange(m) % c.shape[0]                          # (a joker rank with fewer than m keys repeats them)
            fields[g: g + m, r] = c[idx]
            distinct[r] += min(m, c.shape[0])
        out_pairs[g: g + m] = a, b
        g += m
    assert g == groups, f"the search placed {g} of {groups} tables"
    return fields, out_pairs, distinct


def _state_of_fields(variant, fields, pairs, tables, seed):
    """group fields -> a state of len(tables) tables, table i holding group tables[i]; roles i % 3, a multiple of the pair"""
    fl = fields[tables]                                              # [T,15,nf]
    p = pairs[tables]
    T = fl.shape[0]
    mult = 1 + np.arange(T) % np.maximum(1, 20 // np.maximum(p.max(1), 1))
    cols = {k: fl[:, :, i] for i, k in enumerate(KEY_FIELDS[variant])}
    rng = np.random.default_rng(seed)
    for k in FIELD_NAMES:
        cols.setdefault(k, rng.integers(0, 5, (T, 15)))              # (fields the variant's face does not read)
    return state_from_fields(np.arange(T) % 3, p[:, 0] * mult, p[:, 1] * mult, noise_seed=seed, **cols)


@functools.lru_cache(maxsize=None)
def full_load(variant, T):
    """(state, info): info = dict(R, W (ranks 0..12, jokers), distinct [15] keys per rank)"""
    R = hash_region(T)
    W = FULL_LOAD_WINDOW[variant]
    fields, pairs, distinct = _clustered(variant, R, T, W, (R - W[0], R - W[1]), seed=10 * variant + (T & 1))
    st = _state_of_fields(variant, fields, pairs, np.arange(T), seed=20 + variant)
    st.setflags(write=False)
    return st, {"R": R, "W": W, "distinct": distinct}


@functools.lru_cache(maxsize=None)
def one_home(variant, layout):
    """(state, info) for T = 1024: 64 groups of 16 tables with equal keys; layout "block": group g = tables 16 g .. 16 g + 15 (one
    block of the mark kernel), "spread": tables g + 64 k (16 different blocks)"""
    T, R = 1024, 2048
    W = ONE_HOME_WINDOW[variant]
    fields, pairs, distinct = _clustered(variant, R, 64, W, (ONE_HOME_FIRST, ONE_HOME_FIRST), seed=30 + variant, per_pair=1)
    t = np.arange(T)
    group = t // 16 if layout == "block" else t % 64
    fl = fields[group]
    cols = {k: fl[:, :, i] for i, k in enumerate(KEY_FIELDS[variant])}
    rng = np.random.default_rng(40 + variant)
    for k in FIELD_NAMES:
        cols.setdefault(k, rng.integers(0, 5, (T, 15)))
    # the same role and raw pair inside a group: the 16 copies are equal in every byte a face reads
    st = state_from_fields(group % 3, pairs[group, 0], pairs[group, 1], noise_seed=41, **cols)
    st.setflags(write=False)
    return st, {"R": R, "W": W, "first": ONE_HOME_FIRST, "group": group, "distinct": distinct}


def tiny(T):
    rng = np.random.default_rng(50 + T)
    f = rng.integers(0, 5, (7, T, 15))
    return state_from_fields(rng.integers(0, 3, T), rng.integers(0, 21, T), rng.integers(0, 21, T), *f, noise_seed=51)


LEFT_EDGES = ((25, 5), (20, 5), (5, 25), (5, 20), (0, 0), (0, 20), (20, 0), (21, 0), (0, 21), (21, 7), (20, 7), (7, 21), (255, 255),
              (255, 1), (1, 255), (25, 25), (20, 20), (21, 21), (255, 0), (0, 255), (4, 1), (5, 6))
COUNT_EDGES = (4, 5, 7, 255)
ROLE_EDGES = (3, 255)


def domain_edges():
    """(state, what): 64 tables; what[t] = (kind, detail).  Every table is the BASE table (role 0, (n1, n2) = (5, 6), fields with
    hand + taken < total on most ranks) with one thing changed, so two tables differ in the bytes named and nowhere else a face
    reads."""
    rng = np.random.default_rng(60)
    T = 64
    base = {k: rng.integers(0, 4, 15) for k in FIELD_NAMES}
    base["hand"], base["taken"] = rng.integers(0, 2, 15), rng.integers(0, 2, 15)
    base["hand"][13], base["taken"][13] = 0, 0                       # a joker rank that keeps its prob slot
    f = {k: np.tile(v, (T, 1)) for k, v in base.items()}
    role, n1, n2 = np.zeros(T, np.int64), np.full(T, 5), np.full(T, 6)
    what = [("base", None)] * T
    t = 0
    for a, b in LEFT_EDGES:
        n1[t], n2[t], what[t] = a, b, ("left", (a, b))
        t += 1
    for k in FIELD_NAMES:
        for v in COUNT_EDGES:
            f[k][t, :] = v
            what[t] = ("count", (k, v))
            t += 1
    for v in ROLE_EDGES:
        role[t], what[t] = v, ("role", v)
        t += 1
    for v in (1, 2):                                                 # the base under the other roles
        role[t], what[t] = v, ("role", v)
        t += 1
    assert t <= T
    return state_from_fields(role, n1, n2, noise_seed=61, **f), what


def in_direct_domain(state):
    """bool [T]: both opponents' card counts <= 20 -- the domain include/ddz_env.h documents for every finder"""
    f = fields_of_state(state)
    return (f["n1"] <= 20) & (f["n2"] <= 20)


def roles_family(variant):
    """T = 1024 for ddz_q_roles_rows"""
    if variant != 3:
        return full_load(variant, 1024)[0]
    st = every_field()[:1024].copy()
    zero = state_from_fields(np.arange(3), 0, 0, 0, 0, noise_seed=70)        # code 0 on every rank, roles 0 / 1 / 2
    full = state_from_fields(np.arange(3), 7, 9, 4, 4, 4, 4, 4, 4, 4, noise_seed=71)   # the largest code on every rank
    st[0:3], st[3:6] = zero, full
    return st


def family(name, variant, T=None):
    """the state of a family for a finder variant (1, 2 hashed; 3 direct)"""
    if name == "every_field":
        return every_field()
    if name == "chunk_edges":
        assert variant == 3
        return chunk_edges()
    if name == "full_load":
        assert variant in (1, 2)
        return full_load(variant, T or 1024)[0]
    if name in ("one_home_block", "one_home_spread"):
        assert variant in (1, 2)
        return one_home(variant, name[9:])[0]
    if name == "tiny":
        return tiny(T or 37)
    if name == "domain_edges":
        return domain_edges()[0]
    if name == "roles":
        return roles_family(variant)
    raise KeyError(name)
