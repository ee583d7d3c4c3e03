"""CPU: the builder of tests/shared_row_states.py against itself, the finders' keys against face_columns over the whole field
domain (equal key => bit-identical column, different key => a different column or a different rank), face_columns against the
CPU oracle's observe, occupied_slots against a sequential linear-probing simulation, and the comparisons that
tests/test_gpu_shared_row_finders.py applies to the device's output against numpy stand-ins with one word wrong."""
import numpy as np
import pytest

import shared_row_states as S

TILE = 128                                    # rows per fc1 tile (ddz_q_fc1_tile_rows: the segments' alignment)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- the builder against itself ---------------------------------------------------------------------------------------------
def test_fields_read_back_from_the_packed_bytes():
    rng = np.random.default_rng(0)
    T = 300
    role = rng.choice([0, 1, 2, 3, 255], T)
    n1, n2 = rng.integers(0, 256, T), rng.integers(0, 256, T)
    f = {k: rng.integers(0, 256, (T, 15)) for k in S.FIELD_NAMES}
    st = S.state_from_fields(role, n1, n2, **f)
    assert st.shape == (T, 11, 16) and st.dtype == np.uint8
    g = S.fields_of_state(st)
    assert np.array_equal(g["role"], role) and np.array_equal(g["eff"], np.where(role > 2, 0, role))
    assert np.array_equal(g["n1"], n1) and np.array_equal(g["n2"], n2)
    for k in S.FIELD_NAMES:
        assert np.array_equal(g[k], f[k]), k
    # the noise in the bytes no face reads changes no key and no column
    st2 = S.state_from_fields(role, n1, n2, noise_seed=99, **f)
    assert not np.array_equal(st, st2)
    for v in (1, 2, 3):
        assert np.array_equal(S.finder_key(st, v), S.finder_key(st2, v))
        assert np.array_equal(_bits(S.face_columns(st, v)), _bits(S.face_columns(st2, v)))


def test_every_field_meets_its_description():
    st = S.every_field()
    f = S.fields_of_state(st)
    assert st.shape[0] == 1250 and set(f["role"].tolist()) == {0, 1, 2}
    for r in range(15):
        combos = ((f["hand"][:, r] * 5 + f["taken"][:, r]) * 5 + f["b1"][:, r]) * 5 + f["b2"][:, r]
        assert np.unique(combos).size == 625
        for k in S.FIELD_NAMES:
            assert set(f[k][:, r].tolist()) == {0, 1, 2, 3, 4}, (k, r)
    raw = set(zip(f["n1"].tolist(), f["n2"].tolist()))
    assert raw == {(a, b) for a in range(21) for b in range(21)}           # every canonical pair and all its multiples
    for p in raw:
        assert len({int(r) for r, q in zip(f["role"], zip(f["n1"].tolist(), f["n2"].tolist())) if q == p}) >= 2


def test_chunk_edges_meets_its_description():
    st = S.chunk_edges()
    assert st.shape[0] <= 4096
    f = S.fields_of_state(st)
    assert f["n1"].max() <= 20 and f["n2"].max() <= 20 and max(f[k].max() for k in S.FIELD_NAMES) <= 4
    key = S.direct_key(st)
    for r in range(15):
        joker = r >= 13
        codes = np.unique(key[:, r]) - r * S.QSH_COLS
        valid = S.valid_codes(joker)
        assert np.isin(codes, valid).all()
        have = set(codes.tolist())
        # both sides of every chunk boundary: the nearest valid codes, so nothing valid lies between them and the boundary
        for c in range(1, S.QSH_CPR):
            below, above = valid[valid < c * S.QSH_CHUNK].max(), valid[valid >= c * S.QSH_CHUNK].min()
            assert int(below) in have and int(above) in have, (r, c)
        assert 0 in have and S.LARGEST_CODE in have                          # ... of every rank: so of adjacent ranks
        per_chunk = np.bincount(codes // S.QSH_CHUNK, minlength=S.QSH_CPR)
        assert (per_chunk > 0).all()                                          # the last 21 chunks among them
        last = valid[valid >= (S.QSH_CPR - 1) * S.QSH_CHUNK]
        assert last.size == 2 and set(last.tolist()) <= have                  # the partial last chunk: all that is valid
        assert S.QSH_COLS - (S.QSH_CPR - 1) * S.QSH_CHUNK < S.QSH_CHUNK       # (it is partial)
        for c in range(3):                                                    # three consecutive chunks, every valid code
            lo, hi = c * S.QSH_CHUNK, (c + 1) * S.QSH_CHUNK
            want = valid[(valid >= lo) & (valid < hi)]
            assert np.array_equal(codes[(codes >= lo) & (codes < hi)], want) and want.size > S.QSH_CHUNK // 2
            quarter = np.bincount((want - lo) // 512, minlength=4)            # 512 keys per wave of the assign kernel
            assert (quarter > 128).all()                                      # all four waves carry


@pytest.mark.parametrize("T", [1024, 1025])
@pytest.mark.parametrize("variant", [1, 2])
def test_full_load_meets_its_description(variant, T):
    st, info = S.full_load(variant, T)
    R, W = info["R"], info["W"]
    assert st.shape[0] == T and R == S.hash_region(T) == (2048 if T == 1024 else 4096)
    assert W[0] <= 64 and W[1] <= (256 if variant == 1 else 16)               # the caps of the family
    assert S.FULL_LOAD_WINDOW[variant] == W
    words = S.hash_key(st, variant)
    f = S.fields_of_state(st)
    assert set(f["role"].tolist()) == {0, 1, 2} and f["n1"].max() <= 20 and f["n2"].max() <= 20
    for r in range(15):
        w = W[r >= 13]
        home = S.home_slot(words[:, r], R)
        assert home.min() >= R - w and home.max() < R, r
        distinct = np.unique(words[:, r]).size
        assert distinct == info["distinct"][r]
        if r < 13:
            assert distinct == T
            if T == 1024:
                assert 2 * distinct == R                                      # the documented worst load, exactly
        else:
            assert distinct >= w and 2 * distinct >= T
        occ = S.occupied_slots(words[:, r], R)
        assert occ.min() == 0 and occ.min() < home.min()                      # the cluster wraps
        assert distinct - w >= 200                                            # ... and probes run for hundreds of slots


@pytest.mark.parametrize("layout", ["block", "spread"])
@pytest.mark.parametrize("variant", [1, 2])
def test_one_home_meets_its_description(variant, layout):
    st, info = S.one_home(variant, layout)
    assert st.shape[0] == 1024 and info["R"] == 2048
    W = info["W"]
    assert W == ((1, 1) if variant == 2 else S.ONE_HOME_WINDOW[1]) and W[0] <= 8 and W[1] <= 16
    words = S.hash_key(st, variant)
    for r in range(15):
        u, inv, cnt = np.unique(words[:, r], return_inverse=True, return_counts=True)
        assert u.size == 64 and (cnt == 16).all()
        home = S.home_slot(u, 2048)
        w = W[r >= 13]
        assert home.min() >= info["first"] and home.max() < info["first"] + w
        # the family cannot degenerate: 64 keys on w home slots form ONE run of 64 slots, so the keys are displaced from
        # their homes by at least 0 + 1 + ... + 63 - 64 (w - 1) slots in all (1,056 for w = 16: 16 per key and more)
        occ = S.occupied_slots(u, 2048)
        assert occ.max() - occ.min() == 63
        assert int(occ.sum() - home.sum()) >= 2016 - 64 * (w - 1) >= 1056
        blocks = np.arange(1024) // 16                                        # tables per 256-thread block of the mark kernel
        for k in range(64):
            b = np.unique(blocks[inv.reshape(-1) == k])
            assert b.size == (1 if layout == "block" else 16)
    # the 16 copies are equal in every byte a face reads
    cols = S.face_columns(st, variant)
    g = info["group"]
    for k in range(64):
        assert (_bits(cols[g == k]) == _bits(cols[g == k][:1])).all()


def test_tiny_domain_edges_and_roles_meet_their_descriptions():
    for T in (1, 37):
        st = S.tiny(T)
        f = S.fields_of_state(st)
        assert st.shape[0] == T and f["n1"].max() <= 20 and max(f[k].max() for k in S.FIELD_NAMES) <= 4
    st, what = S.domain_edges()
    assert st.shape[0] == 64
    f = S.fields_of_state(st)
    for k in S.FIELD_NAMES:
        for v in (5, 7, 255):
            assert ((f[k] == v).all(1)).any(), (k, v)
    assert {3, 255} <= set(f["role"].tolist())
    for v in (0, 20, 21, 25, 255):
        assert v in f["n1"] and v in f["n2"]
    a, b = what.index(("left", (25, 5))), what.index(("left", (20, 5)))
    dk, cols = S.direct_key(st), S.face_columns(st, 3)
    assert dk[a, 13] == dk[b, 13] and not np.array_equal(_bits(cols[a, 13]), _bits(cols[b, 13]))   # outside the direct domain
    assert cols[a, 13, 16] == np.float32(25) / np.float32(30) and cols[b, 13, 16] == np.float32(0.8)   # (plane 4, slot 0)
    assert not S.in_direct_domain(st)[a] and S.in_direct_domain(st)[b]
    for v in (1, 2):
        hk = S.hash_key(st, v)
        assert hk[a, 13] == hk[b, 13]                                         # the hashed key: the same domain, the same alias
        assert hk[b, 13] == hk[what.index(("left", (4, 1))), 13]            # ... and (20, 5) reduced to (4, 1)
    for v in (1, 2, 3):
        st = S.roles_family(v)
        assert st.shape[0] == 1024
    f = S.fields_of_state(st)
    key = S.direct_key(st)
    for role in range(3):
        m = f["role"] == role
        assert (key[m, 0] == 0).any() and (key[m, 14] == 14 * S.QSH_COLS + S.LARGEST_CODE).any()
        assert 14 * S.QSH_COLS + S.LARGEST_CODE < S.QSH_KEYS <= 15 * S.QSH_COLS


# ---- the keys' claim over the whole field domain --------------------------------------------------------------------------------
ONE = np.float32(1).view(np.uint32)


def _distinct_rows(c):
    """the number of distinct rows of c (uint32 [n, m], m <= 36), exactly: the positions that hold only 0.0f / 1.0f are packed
    into one word, the others two to a word, and the words are sorted lexicographically"""
    binary = ((c == 0) | (c == ONE)).all(0)
    words = [((c[:, binary] == ONE) @ (np.int64(1) << np.arange(int(binary.sum()), dtype=np.int64)))]
    rest = c[:, ~binary].astype(np.int64)
    rest = rest[:, [i for i in range(rest.shape[1]) if not any((rest[:, i] == rest[:, k]).all() for k in range(i))]]
    for i in range(0, rest.shape[1], 2):
        words.append(rest[:, i] << 32 | (rest[:, i + 1] if i + 1 < rest.shape[1] else 0))
    order = np.lexsort(words)
    new = np.zeros(c.shape[0] - 1, bool)
    for w in words:
        new |= w[order][1:] != w[order][:-1]
    return int(new.sum()) + 1


def _claim(keys, cols):
    """equal key => bit-identical column; different key => a different column (keys [n], cols [n, 4 P] of ONE rank)"""
    order = np.argsort(keys, kind="stable")
    k, c = keys[order], _bits(cols)[order]
    same = k[1:] == k[:-1]
    assert (c[1:][same] == c[:-1][same]).all(), "two columns under one key"
    reps = c[np.concatenate([[True], ~same])]                                  # one column per distinct key
    assert _distinct_rows(reps) == reps.shape[0], "one column under two keys"
    return reps.shape[0]


def test_distinct_rows_counts_exactly():
    rng = np.random.default_rng(2)
    c = _bits(rng.choice(np.array([0, 1, 0.8, 0.2, 0.5], np.float32), (5000, 4)))
    assert _distinct_rows(c) == np.unique(c, axis=0).shape[0] < 5000


def _all_combos(nf):
    return np.stack(S._digits(np.arange(5 ** nf), nf), 1)


def test_direct_key_claim_over_its_whole_domain():
    """all 625 x 441 (fields 0..4, card counts 0..20) on a rank < 13 and on a joker rank"""
    combos = np.repeat(_all_combos(4), 441, 0)
    pair = np.tile(np.arange(441), 625)
    cols = {k: combos[:, i][:, None] for i, k in enumerate(S.KEY_FIELDS[3])}
    st = S.state_from_fields(np.arange(combos.shape[0]) % 3, pair // 21, pair % 21, hm1=3, h0=1, hp1=2, **cols)
    key, face = S.direct_key(st), S.face_columns(st, 3)
    for r in (5, 13):
        n = _claim(key[:, r], face[:, r])
        assert n == S.valid_codes(r >= 13).size                                # every valid code, no other
        assert key[:, r].min() == r * S.QSH_COLS and key[:, r].max() == r * S.QSH_COLS + S.LARGEST_CODE


HASH_PAIRS = ((20, 5), (4, 1), (5, 1), (0, 0), (0, 9), (9, 0), (20, 20), (1, 1), (20, 19), (19, 20), (17, 20), (12, 6), (2, 1),
              (1, 2), (20, 10), (7, 3), (3, 7), (0, 20))


@pytest.mark.parametrize("variant", [1, 2])
def test_hashed_key_claim_every_field_combination(variant):
    """every combination of the key fields in 0..4 x 18 (n1, n2) pairs of the domain"""
    nf = len(S.KEY_FIELDS[variant])
    combos = _all_combos(nf)
    n = combos.shape[0]
    keys, faces = [], []
    for a, b in HASH_PAIRS:
        cols = {k: combos[:, i][:, None] for i, k in enumerate(S.KEY_FIELDS[variant])}
        st = S.state_from_fields(np.arange(n) % 3, a, b, **cols)
        keys.append(S.hash_key(st, variant)[:, [5, 13]])
        faces.append(S.face_columns(st, variant)[:, [5, 13]])
    keys, faces = np.concatenate(keys), np.concatenate(faces)
    assert int(keys.max()) - 1 < 1 << S.hash_key_bits(variant) and S.hash_key_bits(variant) == (28 if variant == 1 else 34)
    for i in range(2):
        _claim(keys[:, i], faces[:, i])


@pytest.mark.parametrize("variant", [1, 2])
def test_hashed_key_claim_every_pair_of_the_domain(variant):
    """all 21 x 21 (n1, n2) pairs of the domain x 270 field combinations (18 per rank, count bytes up to 255 among them), every
    pair under each of the role bytes 0, 1, 2, 3, 255"""
    rng = np.random.default_rng(variant)
    pair = np.tile(np.arange(441), 5)
    role = np.repeat([0, 1, 2, 3, 255], 441)
    seen = 0
    for rnd in range(18):
        cols = {k: np.tile(rng.choice([0, 1, 2, 3, 4, 4, 5, 255], 15), (pair.size, 1)) for k in S.FIELD_NAMES}
        if rnd % 2 == 0:
            cols["hand"], cols["taken"] = cols["hand"] * 0, np.minimum(cols["taken"], 1) * (np.arange(15) < 13)   # open prob slots
        st = S.state_from_fields(role, pair // 21, pair % 21, **cols)
        key, face = S.hash_key(st, variant), S.face_columns(st, variant)
        for r in range(15):
            _claim(key[:, r], face[:, r])
            seen += 1
    assert seen >= 256


def test_canonical_pair_claim():
    """fp32(n) / fp32(n1 + n2) is the same float for every multiple of a reduced pair over the 21 x 21 pairs of the documented
    domain, and different reduced pairs give different floats; outside it the saturation aliases: (25, 5) and (20, 5)"""
    n1, n2 = np.divmod(np.arange(441), 21)
    a, b = S._reduced(n1, n2)
    s = n1 + n2 > 0
    with np.errstate(invalid="ignore"):
        for n, c in ((n1, a), (n2, b)):
            got = n.astype(np.float32) / (n1 + n2).astype(np.float32)
            want = c.astype(np.float32) / (a + b).astype(np.float32)
            assert np.array_equal(_bits(got[s]), _bits(want[s]))
        fr = np.stack([a.astype(np.float32) / (a + b).astype(np.float32), b.astype(np.float32) / (a + b).astype(np.float32)], 1)[s]
    code = (a * 21 + b)[s]
    assert np.unique(_bits(fr).view([("", np.uint32)] * 2)).size == np.unique(code).size == S.canonical_pairs().shape[0] - 1
    assert np.float32(25) / np.float32(30) != np.float32(20) / np.float32(25)  # what the saturation at 20 aliases


# ---- face_columns against the oracle ------------------------------------------------------------------------------------------
def _families():
    out = [("every_field", v, None) for v in (1, 2, 3)] + [("chunk_edges", 3, None)]
    out += [("full_load", v, T) for v in (1, 2) for T in (1024, 1025)]
    out += [(n, v, None) for v in (1, 2) for n in ("one_home_block", "one_home_spread")]
    out += [("tiny", v, T) for v in (1, 2, 3) for T in (1, 37)] + [("domain_edges", v, None) for v in (1, 2, 3)]
    out += [("roles", v, None) for v in (1, 2, 3)]
    return out


@pytest.mark.parametrize("name,variant,T", _families())
def test_face_columns_equal_the_oracles_observe(oracle, name, variant, T):
    st = S.family(name, variant, T)
    st = st[st[:, S.F_META, 0] <= 2]                                          # (the oracle does not fold a role byte above 2)
    env = oracle.OracleEnv(st.shape[0], seed=1)
    env.state[:] = st.reshape(-1)
    assert np.array_equal(_bits(env.observe(variant)), _bits(S.face(st, variant)))


# ---- occupied_slots against a sequential simulation -------------------------------------------------------------------------------
def _insert_sequentially(words, R):
    """linear probing, one insert after the other: word -> slot"""
    table, where = {}, {}
    for w in words.tolist():
        if w in where:
            continue
        pos = int(S.home_slot(np.array([w], np.uint64), R)[0])
        while pos in table:
            pos = (pos + 1) & (R - 1)
        table[pos], where[w] = w, pos
    return where


def _orders(words, seed):
    rng = np.random.default_rng(seed)
    return [words, words[::-1], words[rng.permutation(words.size)]]


@pytest.mark.parametrize("variant", [1, 2])
def test_occupied_slots_equal_a_sequential_simulation(variant):
    cases = [(S.hash_key(S.full_load(variant, 1024)[0], variant), 2048), (S.hash_key(S.full_load(variant, 1025)[0], variant), 4096),
             (S.hash_key(S.one_home(variant, "spread")[0], variant), 2048), (S.hash_key(S.every_field(), variant), 4096)]
    for words, R in cases:
        for r in (0, 7, 14):
            want = S.occupied_slots(words[:, r], R)
            for order in _orders(words[:, r], r):
                assert np.array_equal(np.sort(list(_insert_sequentially(order, R).values())), want)


# ---- the comparisons reject a wrong word ------------------------------------------------------------------------------------------
def _standin(state, variant, order_seed=0):
    """what a correct finder may return: (keys, inst, rows, rep, seg, region)"""
    T = state.shape[0]
    keys = S.finder_key(state, variant)
    inst = 16 * np.arange(T)[:, None] + np.arange(15)[None, :]
    region = None if variant == 3 else S.hash_region(T)
    seg = S.seg_words([np.unique(keys[:, r]).size for r in range(15)], TILE)
    cap = int(seg[15]) + 2 * TILE
    rows, rep = np.full((T, 16), -1, np.int64), np.full(cap, -1, np.int64)
    for r in range(15):
        if variant == 3:
            u, first, inv = np.unique(keys[:, r], return_index=True, return_inverse=True)
            rows[:, r], rep[seg[r]: seg[r] + u.size] = seg[r] + inv.reshape(-1), inst[first, r]
        else:
            order = _orders(keys[:, r], order_seed)[2]
            where = _insert_sequentially(order, region)
            rank_of_slot = {s: i for i, s in enumerate(sorted(where.values()))}
            rows[:, r] = [seg[r] + rank_of_slot[where[w]] for w in keys[:, r].tolist()]
            for t in range(T - 1, -1, -1):
                rep[rows[t, r]] = inst[t, r]
    return keys, inst, rows, rep, seg, region


def _check(s, **kw):
    keys, inst, rows, rep, seg, region = (kw.get(k, v) for k, v in zip(("keys", "inst", "rows", "rep", "seg", "region"), s))
    return S.check_finder(keys, rows, rep, seg, TILE, keys, ordered=region is None, region=region)


@pytest.mark.parametrize("variant", [3, 1, 2])
def test_the_finder_comparison_rejects_a_wrong_word(variant):
    state = S.every_field() if variant == 3 else S.full_load(variant, 1024)[0]
    s = _standin(state, variant)
    keys, _, rows, rep, seg, _ = s
    _check(s)
    if variant != 3:
        _check(_standin(state, variant, order_seed=5))                        # another insertion order: other rows, still right
    r = 4
    t0 = 0
    t1 = int(np.flatnonzero(keys[:, r] != keys[t0, r])[0])
    bad = rows.copy()                                                         # two rows swapped between tables with different keys
    bad[t0, r], bad[t1, r] = rows[t1, r], rows[t0, r]
    with pytest.raises(AssertionError):
        _check(s, rows=bad)
    bad = rep.copy()                                                          # one rep pointed at an instance of another key
    bad[rows[t0, r]] = 16 * t1 + r
    with pytest.raises(AssertionError):
        _check(s, rep=bad)
    bad = seg.copy()                                                          # one segment start moved by a tile
    bad[r] += TILE
    with pytest.raises(AssertionError):
        _check(s, seg=bad)
    bad = rows.copy()
    bad[:, 15] = 0
    with pytest.raises(AssertionError):
        _check(s, rows=bad)
    bad = rep.copy()                                                          # a padding row with a representative
    bad[int(seg[15]) + 1] = 0
    with pytest.raises(AssertionError):
        _check(s, rep=bad)
    if variant != 3:
        # a row numbering that is no slot order, on a sparse region (every_field): the rows on both sides of an EMPTY slot
        # exchanged -- the upper key would sit below its home, reached only round the ring over empty slots
        s2 = _standin(S.every_field(), variant)
        keys2, _, rows2, rep2, seg2, region2 = s2
        _check(s2)
        occ = S.occupied_slots(keys2[:, r], region2)
        i = int(np.flatnonzero(np.diff(occ) > 1)[0])                          # (asserted by the index: such a gap exists)
        a, b = int(seg2[r]) + i, int(seg2[r]) + i + 1
        bad_rows, bad_rep = rows2.copy(), rep2.copy()
        bad_rows[:, r] = np.where(rows2[:, r] == a, b, np.where(rows2[:, r] == b, a, rows2[:, r]))
        bad_rep[a], bad_rep[b] = rep2[b], rep2[a]
        with pytest.raises(AssertionError, match="not reached from its key's home"):
            _check(s2, rows=bad_rows, rep=bad_rep)


def test_the_need_comparison_rejects_a_wrong_word():
    state = S.every_field()
    _, _, rows, rep, seg, _ = _standin(state, 3)
    rng = np.random.default_rng(8)
    ri = np.where(rng.random((state.shape[0], 64)) < 0.5, 7, -1)
    ri[:, 54:] = -1
    ri2, drep, cnt, dseg, n = S.expected_need(ri, rows, seg, TILE)
    assert n == dseg[15] and (ri2[:, :54] >= 0).sum() == (ri[:, :54] >= 0).sum()
    S.check_need(ri, rows, seg, TILE, ri2, drep, cnt, dseg)
    k = int(np.flatnonzero((drep >= 0) & ((drep & 3) < 3))[0])
    bad = drep.copy()                                                         # one drep entry off by one count
    bad[k] += 1
    with pytest.raises(AssertionError):
        S.check_need(ri, rows, seg, TILE, ri2, bad, cnt, dseg)
    bad = cnt.copy()
    bad[k] += 1
    with pytest.raises(AssertionError):
        S.check_need(ri, rows, seg, TILE, ri2, drep, bad, dseg)
    bad = ri2.copy()
    t, c = np.argwhere(ri2 >= 0)[0]
    bad[t, c] += 1
    with pytest.raises(AssertionError):
        S.check_need(ri, rows, seg, TILE, bad, drep, cnt, dseg)
    bad = dseg.copy()
    bad[3] += TILE
    with pytest.raises(AssertionError):
        S.check_need(ri, rows, seg, TILE, ri2, drep, cnt, bad)
    # the overflow statement: a capacity of 15 tiles against more pairs than that
    cap = 15 * TILE
    o_ri2, o_drep, o_cnt, o_dseg, o_n = S.expected_need(ri, rows, seg, TILE, capacity=cap)
    assert dseg[15] > cap and o_dseg[33] == 1 and o_dseg[15] == o_n == cap and o_dseg[32] == dseg[32]
    assert o_ri2.max() < cap and np.array_equal(o_ri2[o_ri2 >= 0], ri2[o_ri2 >= 0]) and np.array_equal(o_drep, drep[:cap])
    assert (o_ri2 >= 0).sum() < (ri2 >= 0).sum()
