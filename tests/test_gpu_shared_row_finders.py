"""GPU (-m gpu): the shared-row finders ALONE on imported states built key by key (tests/shared_row_states.py; pinned by
tests/test_shared_row_states_cpu.py): ddz_q_shared_rows, ddz_q_shared_rows_hashed, ddz_q_roles_rows, ddz_q_shared_need and
ddz_q_roles_need through engine.py's wrappers, their integer outputs compared exactly with the numpy statement, and H0 / the D
rows' first layer of EVERY table against the fp64 statement of tests/q_reference.py evaluated from the table's OWN columns.

What play from a fresh deal never reaches and these states do: the last 21 chunks of a rank of the direct table (the partial
last one too), the last key of a rank / slot beside the first key of the next, chunks in which all four waves of the assign scan
carry; a hashed region at load 1/2, probe chains that wrap from the last slot of a region to its first and run for hundreds of
slots, 64 keys on one home slot; workspaces that are not zero on entry; the overflow path of ddz_q_shared_need.

Finder / kernels                                   pinned by
  ddz_q_shared_rows (k_qs_mark, count, seg, ...)   test_direct_finder        rows, rep, seg word for word; twice
  ddz_q_shared_rows_hashed (k_qs_hmark<V>, ...)    test_hashed_finder        seg exact, rows <-> keys, slot order, wrap; 3 calls + a side stream
  ddz_q_roles_rows (k_qs_[h]mark_roles, ...)       test_roles_finder         per slot partition; slot[t]; rule tables; one-slot map
  ddz_q_shared_need / _roles_need (k_qd_*)         test_shared_need, test_roles_need, test_shared_need_overflow
  the values an aliased row would corrupt          test_values_of_every_table (+ the control: two rows exchanged must fail)
  the documented domain of the keys                test_domain_edges
Every finder call runs once with its workspace zero-filled and once pre-filled with 0xA5 bytes; every output buffer carries a
sentinel tail that must come back untouched."""
import importlib

import numpy as np
import pytest
import torch

import q_reference as qr
import shared_row_states as S
import test_gpu_q_kernels as qk
from test_gpu_q_kernels import _stop_after_a_device_fault  # noqa: F401  (autouse here too: a device fault ends the session)

pytestmark = pytest.mark.gpu
H = qr.H
TAIL = 128                                    # sentinel words behind every output buffer
FILLS = (0, 0xA5)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


@pytest.fixture(scope="module")
def glue():
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


@pytest.fixture(scope="module")
def E():
    return importlib.import_module("doudizhu-rl_amd.engine")


def _dev():
    return torch.device("cuda:0")


def _full(n, fill, dt):
    return torch.full((n,), fill, dtype=dt, device=_dev())


def _env(pkg, state):
    env = pkg.BatchedEnv(state.shape[0], seed=3, device=_dev())
    env.reset()
    env.state_import(torch.from_numpy(np.ascontiguousarray(state).reshape(-1).copy()))
    return env


def _scap(T, variant, tile):
    most = min(15 * T, S.QSH_KEYS) if variant == 3 else 15 * T
    return (most + 15 * tile + tile - 1) // tile * tile


def _find(env, E, variant, tile, fill, net_of_role=None):
    """one finder call on buffers with sentinel tails: host copies of rows [T,16], rep [N * scap], seg [N,40] (+ slot [T])"""
    T = env.T
    N = 1 if net_of_role is None else max(net_of_role) + 1
    scap = _scap(T, variant, tile)
    rows = torch.full((T + TAIL // 16, 16), 77777, dtype=torch.int32, device=_dev())
    rep, seg, slot = _full(N * scap + TAIL, 55555, torch.int32), _full(N * 40 + TAIL, 33333, torch.int32), _full(T + TAIL, 99, torch.int8)
    if net_of_role is None:
        nbytes = E.q_shared_ws_bytes() if variant == 3 else E.q_shared_hash_ws_bytes(T)
    else:
        nbytes = E.q_roles_ws_bytes(T, variant, N)
    ws = _full(nbytes + TAIL, fill, torch.uint8)
    ws[nbytes:] = 0x3C
    if net_of_role is None:
        env.q_shared_rows(ws[:nbytes], scap, rows[:T], rep[: scap], seg[:40], variant=variant)
    else:
        env.q_roles_rows(variant, net_of_role, N, ws[:nbytes], scap, rows[:T], rep[: N * scap], seg[: N * 40], slot[:T])
    torch.cuda.synchronize()
    assert bool((rows[T:] == 77777).all()) and bool((rep[N * scap:] == 55555).all()) and bool((seg[N * 40:] == 33333).all())
    assert bool((ws[nbytes:] == 0x3C).all()) and bool((slot[T:] == 99).all()), "a write outside a buffer"
    assert env.status() == 0
    return {"rows": rows[:T].cpu().numpy().astype(np.int64), "rep": rep[: N * scap].cpu().numpy().astype(np.int64),
            "seg": seg[: N * 40].cpu().numpy().reshape(N, 40), "slot": slot[:T].cpu().numpy().astype(np.int64), "scap": scap, "N": N,
            "dev": {"rows": rows[:T], "rep": rep[: N * scap], "seg": seg[: N * 40]}}


def _check_single(state, variant, out, tile):
    keys = S.finder_key(state, variant)
    region = None if variant == 3 else S.hash_region(state.shape[0])
    return S.check_finder(keys, out["rows"], out["rep"], out["seg"][0], tile, keys, ordered=variant == 3, region=region)


def _row_sets(state, variant, out):
    """key -> row is a function both ways (per rank); the relation itself may differ from call to call of the hashed finder"""
    keys = S.finder_key(state, variant)
    return [np.unique(np.stack([keys[:, r].astype(np.int64), out["rows"][:, r]], 1), axis=0).shape[0] for r in range(15)]


DIRECT = [("every_field", None), ("chunk_edges", None), ("tiny", 1), ("tiny", 37), ("domain_edges", None)]
HASHED = DIRECT[:1] + [("full_load", 1024), ("full_load", 1025), ("one_home_block", None), ("one_home_spread", None)] + DIRECT[2:]


@pytest.mark.parametrize("name,T", DIRECT)
def test_direct_finder(pkg, E, glue, name, T):
    """rows[t][r] exactly the position of direct_key(t, r) among the rank's sorted distinct keys, rows[:, 15] = -1, rep[row] an
    instance with the row's key, rep = -1 on every padding row and behind seg[15], seg[0..33] as computed; a second call and a
    call on a workspace full of 0xA5 give identical words"""
    tile = glue.fc_tile()
    state = S.family(name, 3, T)
    env = _env(pkg, state)
    want_rows, _, want_seg = S.expected_direct(state, tile)
    first = None
    for fill in FILLS + (0,):
        out = _find(env, E, 3, tile, fill)
        _check_single(state, 3, out, tile)
        assert np.array_equal(out["rows"], want_rows) and np.array_equal(out["seg"][0][:34], want_seg[:34]) and out["seg"][0][33] == 0
        first = first or out
        assert np.array_equal(out["rows"], first["rows"]) and np.array_equal(out["seg"][0][:34], first["seg"][0][:34])
        key = S.direct_key(state).reshape(-1)
        live = out["rep"] >= 0                                                # (rep itself may name another instance of the key)
        assert np.array_equal(live, first["rep"] >= 0)
        assert np.array_equal(key[(out["rep"][live] >> 4) * 15 + (out["rep"][live] & 15)],
                              key[(first["rep"][live] >> 4) * 15 + (first["rep"][live] & 15)])
    if name == "chunk_edges":                                                 # the family did occupy what it is there for
        codes = S.direct_key(state) % S.QSH_COLS
        assert (np.bincount((codes // S.QSH_CHUNK).reshape(-1), minlength=S.QSH_CPR) > 0).all()


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("name,T", HASHED)
def test_hashed_finder(pkg, E, glue, name, T, variant):
    """seg exactly as computed from the distinct keys per rank; per rank rows <-> keys a bijection inside the rank's segment;
    hash_key(rep[row]) the row's key; padding rows rep = -1; the i-th row of a rank sits in the i-th occupied slot of
    occupied_slots, reached from its key's home over occupied slots only (so no chain left its region); on full_load the
    chains did wrap.  Three calls and one on a side stream, zero and 0xA5 workspaces: the same key <-> row-set relation."""
    tile = glue.fc_tile()
    state = S.family(name, variant, T)
    env = _env(pkg, state)
    R = S.hash_region(state.shape[0])
    side = torch.cuda.Stream()
    sets = None
    for call, fill in enumerate(FILLS + (0, 0xA5)):
        if call == 3:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                out = _find(env, E, variant, tile, fill)
            torch.cuda.current_stream().wait_stream(side)
        else:
            out = _find(env, E, variant, tile, fill)
        _check_single(state, variant, out, tile)
        assert out["seg"][0][33] == 0
        sets = sets or _row_sets(state, variant, out)
        assert _row_sets(state, variant, out) == sets
    if name == "full_load":
        words = S.hash_key(state, variant)
        for r in range(15):
            occ = S.occupied_slots(words[:, r], R)
            assert occ.min() < S.home_slot(words[:, r], R).min()              # the chains really wrapped


def _check_roles(state, variant, net_of_role, out, tile):
    T = state.shape[0]
    slot = S.slot_of_tables(state, net_of_role)
    assert np.array_equal(out["slot"], slot)
    keys = S.finder_key(state, variant)
    region = None if variant == 3 else S.hash_region(T)
    cap = out["scap"]
    rows = out["rows"]
    assert (rows[slot < 0] == -1).all() and (rows[:, 15] == -1).all()        # a rule table owns no row
    for s in range(out["N"]):
        m = slot == s
        rel = rows[m].copy()
        assert ((rel[:, :15] >= s * cap) & (rel[:, :15] < (s + 1) * cap)).all(), "a row outside its slot's partition"
        rel[:, :15] -= s * cap
        S.check_finder(keys[m], rel, out["rep"][s * cap: (s + 1) * cap], out["seg"][s], tile, keys,
                       ordered=variant == 3, region=region)
        assert set((out["rep"][s * cap: (s + 1) * cap][out["rep"][s * cap: (s + 1) * cap] >= 0] >> 4).tolist()) <= set(np.flatnonzero(m).tolist())


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_roles_finder(pkg, E, glue, variant):
    """ddz_q_roles_rows under four role maps: the single-network checks per slot partition, slot[t] = the map of the actor's
    role, rule tables -1 and without a row, no row of slot s outside [s cap, (s + 1) cap); a one-slot map gives the
    single-network words (variant 3) / the single-network relation (1, 2)"""
    tile = glue.fc_tile()
    state = S.roles_family(variant)
    env = _env(pkg, state)
    for m in S.ROLE_MAPS + ([0, 0, 0],):
        for fill in FILLS:
            one = _find(env, E, variant, tile, fill, net_of_role=m)
            _check_roles(state, variant, m, one, tile)
    single = _find(env, E, variant, tile, 0)                                  # (one: the one-slot map [0, 0, 0])
    assert np.array_equal(one["seg"][0][:34], single["seg"][0][:34])
    if variant == 3:
        assert np.array_equal(one["rows"], single["rows"]) and np.array_equal(one["rep"] >= 0, single["rep"] >= 0)
        key = S.direct_key(state)
        f = S.fields_of_state(state)
        for role in range(3):                                                 # the last key of a slot beside the first of the next
            mrole = f["eff"] == role
            assert (key[mrole, 0] == 0).any() and (key[mrole, 14] == S.QSH_KEYS - S.QSH_COLS + S.LARGEST_CODE).any()


# ---- ddz_q_shared_need / ddz_q_roles_need -------------------------------------------------------------------------------------
PATTERNS = ("all", "none", "count4", "jokers", "half")


def _row_index(T, pattern, seed=0):
    ri = np.full((T, 64), -1, np.int32)
    col = np.arange(54)
    if pattern == "all":
        ri[:, :54] = 7
    elif pattern == "count4":
        ri[:, col[(col < 52) & (col % 4 == 3)]] = 0
    elif pattern == "jokers":
        ri[:, 52:54] = 3
    elif pattern == "half":
        ri[:, :54] = np.where(np.random.default_rng(seed).random((T, 54)) < 0.5, 11, -1)
    return ri


def _need(env, E, found, row_index, tile, dcap, fill, roles=False):
    T, N, scap = env.T, found["N"], found["scap"]
    ri = torch.from_numpy(row_index).to(_dev())
    ri2 = torch.full((T + TAIL // 64, 64), 44444, dtype=torch.int32, device=_dev())
    drep, dseg = _full(N * dcap + TAIL, 66666, torch.int32), _full(N * 40 + TAIL, 22222, torch.int32)
    cnt = _full(N * dcap + TAIL, 0xEE, torch.uint8)
    nbytes = E.q_roles_need_ws_bytes(scap, N) if roles else E.q_shared_need_ws_bytes(scap)
    ws = _full(nbytes + TAIL, fill, torch.uint8)
    ws[nbytes:] = 0x3C
    d = found["dev"]
    if roles:
        env.q_roles_need(N, ri, d["rows"], d["seg"], scap, ws[:nbytes], dcap, ri2[:T], drep[: N * dcap], dseg[: N * 40], cnt[: N * dcap])
    else:
        env.q_shared_need(ri, d["rows"], d["seg"], scap, ws[:nbytes], dcap, ri2[:T], drep[:dcap], dseg[:40], cnt[:dcap])
    torch.cuda.synchronize()
    assert bool((ri2[T:] == 44444).all()) and bool((drep[N * dcap:] == 66666).all()) and bool((dseg[N * 40:] == 22222).all())
    assert bool((cnt[N * dcap:] == 0xEE).all()) and bool((ws[nbytes:] == 0x3C).all()), "a write outside a buffer"
    return {"ri2": ri2[:T].cpu().numpy().astype(np.int64), "drep": drep[: N * dcap].cpu().numpy().astype(np.int64),
            "dseg": dseg[: N * 40].cpu().numpy().reshape(N, 40), "cnt": cnt[: N * dcap].cpu().numpy().astype(np.int64)}


def _dcap(T, tile):
    return (54 * T + 15 * tile + tile - 1) // tile * tile


@pytest.mark.parametrize("name,variant", [("every_field", 3), ("every_field", 1), ("full_load", 1), ("full_load", 2)])
def test_shared_need(pkg, E, glue, name, variant):
    """ddz_q_shared_need on a constructed row_index over the finder's rows: the D rows are the distinct (shared row, count)
    pairs in ascending 4 row + c - 1 order inside each rank's segment -- drep, row_cnt, dseg and row_index2 exactly"""
    tile = glue.fc_tile()
    state = S.family(name, variant, 1024)
    env = _env(pkg, state)
    found = _find(env, E, variant, tile, 0)
    T = state.shape[0]
    dcap = _dcap(T, tile)
    for i, (pattern, fill) in enumerate((p, f) for p in PATTERNS for f in FILLS):
        ri = _row_index(T, pattern, seed=i // 2)
        got = _need(env, E, found, ri, tile, dcap, fill)
        n = S.check_need(ri, found["rows"], found["seg"][0], tile, got["ri2"], got["drep"], got["cnt"], got["dseg"][0])
        assert (got["drep"][n:] == -1).all() and (got["cnt"][n:] == 0xEE).all() and got["dseg"][0][33] == 0
        assert np.array_equal(got["ri2"][:, :54] >= 0, ri[:, :54] >= 0) and (got["ri2"][:, 54:] == -1).all()
        if pattern == "none":
            assert n == 0 and got["dseg"][0][32] == 0
        if pattern == "all":
            assert got["dseg"][0][32] > 15 * tile
    assert env.status() == 0


@pytest.mark.parametrize("variant", [3, 2])
def test_roles_need(pkg, E, glue, variant):
    """ddz_q_roles_need: ddz_q_shared_need's statement on every slot's partition (rows and D rows relative to the slot's
    capacities), every column of a rule table -1"""
    tile = glue.fc_tile()
    state = S.roles_family(variant)
    env = _env(pkg, state)
    T = state.shape[0]
    dcap = _dcap(T, tile)
    for i, m in enumerate(([0, 1, 2], [1, -1, 0])):
        found = _find(env, E, variant, tile, 0, net_of_role=m)
        slot, scap = found["slot"], found["scap"]
        for pattern, fill in ((p, f) for p in ("all", "half") for f in FILLS):
            ri = _row_index(T, pattern, seed=5 + i)
            got = _need(env, E, found, ri, tile, dcap, fill, roles=True)
            assert (got["ri2"][slot < 0] == -1).all()
            for s in range(found["N"]):
                msk = slot == s
                rel = found["rows"][msk].copy()
                rel[:, :15] -= s * scap
                r2 = got["ri2"][msk].copy()
                assert ((r2 == -1) | ((r2 >= s * dcap) & (r2 < (s + 1) * dcap))).all()
                r2[r2 >= 0] -= s * dcap
                S.check_need(ri[msk], rel, found["seg"][s], tile, r2, got["drep"][s * dcap: (s + 1) * dcap],
                             got["cnt"][s * dcap: (s + 1) * dcap], got["dseg"][s])
    assert env.status() == 0


def test_shared_need_overflow(pkg, E, glue):
    """the documented minimum capacity of 15 tiles against more (row, count) pairs than that: status bit 1, dseg[33] = 1,
    dseg[15] <= capacity, dseg[32] the true count, every row_index2 < capacity and equal to the unconstrained numbering where
    it is not -1, drep / row_cnt behind the capacity untouched.  The kernels guard this path (the counterpart of ddz_q_need's
    "row capacity too small" test)."""
    tile = glue.fc_tile()
    state = S.every_field()
    env = _env(pkg, state)                                                    # (an env of its own: the status bit stays set)
    found = _find(env, E, 3, tile, 0)
    T, cap = state.shape[0], 15 * tile
    ri = _row_index(T, "all")
    free = S.expected_need(ri, found["rows"], found["seg"][0], tile)
    assert free[4] > cap                                                      # more pairs than the capacity holds
    got = _need(env, E, found, ri, tile, cap, 0xA5)
    assert env.status() & 2
    dseg = got["dseg"][0]
    assert dseg[33] == 1 and dseg[15] <= cap and dseg[32] == free[3][32]
    assert got["ri2"].max() < cap and (got["ri2"] >= 0).any()
    assert np.array_equal(got["ri2"][got["ri2"] >= 0], free[0][got["ri2"] >= 0])
    S.check_need(ri, found["rows"], found["seg"][0], tile, got["ri2"], got["drep"], got["cnt"], dseg, capacity=cap)


# ---- the values ----------------------------------------------------------------------------------------------------------------
def _first_layer_chunked(face, wf, bias, acnt, chunk=64):
    ys, abs_ = [], []
    for lo in range(0, face.shape[0], chunk):
        y, _, ab = qr.first_layer(face[lo: lo + chunk], wf, bias, acnt)
        ys.append(y)
        abs_.append(ab)
    return torch.cat(ys), torch.cat(abs_)


def _values_case(pkg, E, glue, state, variant, swap=None):
    """H0 of every table and the first layer of every D row a table needs, from the finder's rows, against the fp64 value of
    the table's own columns.  swap = (t0, t1, r): the two tables' rows of rank r exchanged before the gather (the control)."""
    tile = glue.fc_tile()
    T, P = state.shape[0], S.PLANES[variant]
    K = qr.wide_width(P)
    env = _env(pkg, state)
    face = env.observe(variant)
    torch.cuda.synchronize()
    assert np.array_equal(face.cpu().numpy().view(np.uint32), S.face(state, variant).view(np.uint32))   # roles > 2 included
    wf, bias, acnt = qk._first_layer_weights(P, 90 + variant, integer=False)
    g = torch.Generator().manual_seed(7 + variant)
    W2x = torch.randn((15, K, H), generator=g).float().double()
    W2x[:, H + 4 * P:] = 0.0
    base = torch.randn(H, generator=g).float().double()
    Y, ab = _first_layer_chunked(face.cpu().double(), wf, bias, acnt)         # [T,15,5,256]
    cols = qr.face_columns(face.cpu())                                        # [T,15,4 P]
    x = torch.cat([Y[:, :, 0], cols, torch.zeros((T, 15, K - H - 4 * P), dtype=torch.float64)], 2)
    xa = torch.cat([ab[:, :, 0], cols.abs(), torch.zeros((T, 15, K - H - 4 * P), dtype=torch.float64)], 2)
    want = base[None, :] + torch.einsum("trk,rko->to", x, W2x)
    wab = base.abs()[None, :] + torch.einsum("trk,rko->to", xa, W2x.abs())
    rk, cnt = S.need_columns()
    ri = _row_index(T, "all")                                                 # the D rows: every (t, r, c)
    dcap = _dcap(T, tile)
    for fill in FILLS:                                                        # both workspaces of both finders zero / 0xA5
        found = _find(env, E, variant, tile, fill)
        scap, d = found["scap"], found["dev"]
        rows = d["rows"]
        if swap:
            t0, t1, r = swap
            rows = rows.clone()
            rows[t0, r], rows[t1, r] = d["rows"][t1, r], d["rows"][t0, r]
        ys, gg, h0 = qk._nan(scap, K), qk._nan(scap, H), qk._nan(T, H)
        pkg.q_features_rows(face, qk._d(wf), qk._d(bias), d["rep"], d["seg"], ys)
        pkg.q_fc1_rows_k(ys, d["seg"], qk._d(W2x), gg)
        pkg.q_gather_h0(gg, rows, h0, base=qk._d(base))
        need = _need(env, E, found, ri, tile, dcap, fill)
        dy = qk._nan(dcap, H)
        pkg.q_features_drows(face, qk._d(wf), qk._d(bias), qk._acnt_dev(acnt), d["rep"], qk._d(need["drep"], torch.int32),
                             qk._d(need["dseg"][0], torch.int32), dy)
        torch.cuda.synchronize()
        assert env.status() == 0
        # the first-layer chain (4 P products, the bias), the K products of the row, the sixteen terms of the gather
        qr.assert_within(h0.cpu(), want, wab, qr.first_layer_terms(P, 0) + K + 16)
        t_, c_ = np.nonzero(need["ri2"][:, :54] >= 0)
        got = dy.cpu()[torch.from_numpy(need["ri2"][t_, c_])]
        tt, rr, cc = torch.from_numpy(t_), torch.from_numpy(rk[c_]), torch.from_numpy(cnt[c_])
        qr.assert_within(got, Y[tt, rr, cc] - Y[tt, rr, 0], ab[tt, rr, cc] + ab[tt, rr, 0], qr.difference_terms(P))


@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("name", ["every_field", "full_load", "domain_edges"])
def test_values_of_every_table(pkg, E, glue, name, variant):
    """the device's own ddz_observe face equals face_columns bit for bit; ddz_q_features_rows -> ddz_q_fc1_rows_k ->
    ddz_q_gather_h0 on the finder's rows gives every table the H0 of its OWN columns, ddz_q_features_drows every needed D row
    the first-layer difference of the needing table's OWN column -- within gamma_n sum |terms| (q_reference.assert_within)"""
    if name == "full_load" and variant == 3:
        state = S.chunk_edges()[:1024]                                        # (the direct table's counterpart)
    else:
        state = S.family(name, variant, 1024)
    state = state[S.in_direct_domain(state)]      # the keys' documented domain: a table outside it may hand ITS column to
                                                  # the tables that share its key
    _values_case(pkg, E, glue, state, variant)


@pytest.mark.parametrize("variant", [1, 3])
def test_values_control_an_aliased_row_is_seen(pkg, E, glue, variant):
    """the control: two tables whose keys of one rank differ get each other's row -- the H0 comparison must fail, so the bound
    is tight enough to see an aliased row"""
    state, what = S.domain_edges()
    dom = np.flatnonzero(S.in_direct_domain(state))
    state = state[dom]
    t0, t1 = (int(np.flatnonzero(dom == what.index(("left", p)))[0]) for p in ((4, 1), (5, 6)))
    r = 13                                                                    # its open slot: 0.8 against 5 / 11
    assert S.finder_key(state, variant)[t0, r] != S.finder_key(state, variant)[t1, r]
    with pytest.raises(AssertionError, match="outside gamma_n"):
        _values_case(pkg, E, glue, state, variant, swap=(t0, t1, r))


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_domain_edges(pkg, E, glue, variant):
    """count bytes 5 / 7 / 255, role bytes 3 / 255, left bytes 0 / 20 / 21 / 25 / 255: for every pair of instances of a rank
    with left bytes <= 20 (the domain include/ddz_env.h documents for every finder), equal row <=> equal column; beyond that
    the row is in its rank's segment (it may be another table's column: (25, 5) shares the row of (20, 5)), status 0, nothing
    written outside the buffers"""
    tile = glue.fc_tile()
    state, what = S.domain_edges()
    env = _env(pkg, state)
    face = env.observe(variant).cpu().numpy()
    assert np.array_equal(face.view(np.uint32), S.face(state, variant).view(np.uint32))
    cols = S.face_columns(state, variant).view(np.uint32)
    dom = S.in_direct_domain(state)
    a, b = what.index(("left", (25, 5))), what.index(("left", (20, 5)))
    for fill in FILLS:
        out = _find(env, E, variant, tile, fill)                              # (status 0 and the sentinel tails: inside)
        seg = _check_single(state, variant, out, tile)                        # (every row inside its rank's segment)
        for r in range(15):
            row = out["rows"][dom, r]
            same_row = row[:, None] == row[None, :]
            same_col = (cols[dom, r][:, None, :] == cols[dom, r][None, :, :]).all(2)
            assert np.array_equal(same_row, same_col), r
        assert out["rows"][a, 13] == out["rows"][b, 13]                        # outside the domain: (25, 5) reads as (20, 5)
        assert seg[33] == 0
