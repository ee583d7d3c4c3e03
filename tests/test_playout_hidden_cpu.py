"""CPU: tests/playout_hidden_reference.py (playout spec v2, hidden hands, on the oracle) -- conservation, independence from
the opponents' rows, uniformity of the redeal, the domain, degenerate pools, and that the exact comparison the GPU tests make
rejects a perturbed world; the serving codec of the plain payload and the exported symbols.  The states are shared with
tests/test_gpu_playout_hidden.py, which holds ddz_playout_worlds / ddz_playout_hidden to the same reference."""
import importlib
import json
import math
import os
import re

import numpy as np
import pytest

import constructed_states as cs
import playout_hidden_cases as hc
import playout_hidden_reference as phr
import playout_reference as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 5


@pytest.fixture(scope="module")
def table(oracle):
    return cs.Table(*oracle.action_table())


@pytest.fixture(scope="module")
def games(oracle):
    st = hc.game_states(oracle)
    W, part, bad = phr.worlds(oracle, st, K, seed=hc.SEED, gid_base=hc.GID_BASE)
    return st, W, part, bad


def test_game_states_cover_the_roles(games, table):
    st, W, part, bad = games
    cs.check_consistent(st, table)
    run = cs.running(st)
    assert run.sum() >= 30 and np.array_equal(part, run) and not bad.any()
    plies = np.array([hc.plies_of(i) for i in range(len(st))])
    assert cs.meta_ply(st)[run].tolist() == plies[run].tolist()
    for depth in hc.DEPTH:
        near = run & (plies >= depth) & (plies < depth + 3)
        assert set(st[near, cs.F_META, cs.M_ROLE].tolist()) == {0, 1, 2}, depth


def test_conservation(games):
    st, W, part, bad = games
    dec = phr.decode(st)
    for t in np.flatnonzero(part):
        run, role, unseen, n_next, n_prev, ok = dec[t]
        assert ok
        for k in range(K):
            nxt, prv = W[t, k, 0].astype(np.int64), W[t, k, 1].astype(np.int64)
            assert np.array_equal(nxt[:15] + prv[:15], unseen), (t, k)
            assert nxt[15] == nxt[:15].sum() == n_next and prv[15] == prv[:15].sum() == n_prev, (t, k)
            copy = phr.with_world(st[t], W[t, k])
            other = [r for r in range(11) if r not in ((role + 1) % 3, (role + 2) % 3)]
            assert np.array_equal(copy[other], st[t][other])              # the actor's hand and every other row
            # a world is a state the engine could be in: hands + taken = the deck
            assert np.array_equal(copy[0:3, :15].astype(np.int64).sum(0) + copy[cs.F_TAKEN, :15], cs.DECK)
    assert not W[~part].any()
    # the true hands are one of the possible worlds, and the redeal is not a copy of them
    true = hc.true_worlds(st, K)[0]
    assert not np.array_equal(true[part], W[part])


def test_worlds_depend_on_gid_k_seed_salt_only(oracle, games):
    st, W, part, bad = games
    t = int(np.flatnonzero(part)[3])
    alone = phr.worlds(oracle, st[t:t + 1], K, seed=hc.SEED, gid_base=hc.GID_BASE + t)[0]
    assert np.array_equal(alone[0], W[t])                                  # gid = gid_base + t, not the position
    assert len({W[t, k].tobytes() for k in range(K)}) > 1                  # k
    for kw in ({"seed": hc.SEED + 1}, {"seed": hc.SEED, "salt": 1}, {"seed": hc.SEED + (1 << 32)}):
        other = phr.worlds(oracle, st[t:t + 1], K, gid_base=hc.GID_BASE + t, **kw)[0]
        assert not np.array_equal(other[0], W[t]), kw
    assert np.array_equal(phr.worlds(oracle, st[t:t + 1], K + 3, seed=hc.SEED, gid_base=hc.GID_BASE + t)[0][0, :K], W[t])


def test_independence_from_the_opponents_rows(oracle, games):
    st, W, part, bad = games
    pick = np.flatnonzero(part)[[0, 1, 2, 13, 14, 30]]                     # depths 0, 12 and 30; short lists among them
    live = st[pick]
    want = phr.playouts_hidden(oracle, live, 2, seed=3, gid_base=5)
    assert want[1][1] > 0 and want[1][2] == 0
    open_live = pr.playouts(oracle, live, 2, seed=3, gid_base=5)
    for fill in (0, np.random.default_rng(1)):
        other = hc.strip_opponents(live, fill)
        assert not np.array_equal(other, live)
        assert np.array_equal(phr.worlds(oracle, other, K, seed=hc.SEED)[0], phr.worlds(oracle, live, K, seed=hc.SEED)[0])
        got = phr.playouts_hidden(oracle, other, 2, seed=3, gid_base=5)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    # ... and the test discriminates: the open reference does read those rows
    emptied = pr.playouts(oracle, hc.strip_opponents(live, 0), 2, seed=3, gid_base=5)
    assert not np.array_equal(emptied[0], open_live[0]) and not np.array_equal(emptied[1], open_live[1])


def test_the_loop_is_spec_v1_on_the_world(oracle, games):
    """with every world = the hands the opponents really hold, playouts_hidden IS playout_reference.playouts"""
    st, W, part, bad = games
    live = st[np.flatnonzero(part)[[1, 2, 13, 14, 30]]]
    got = phr.playouts_hidden(oracle, live, 3, seed=11, gid_base=2 ** 32 + 7, salt=4, the_worlds=hc.true_worlds(live, 3))
    want = pr.playouts(oracle, live, 3, seed=11, gid_base=2 ** 32 + 7, salt=4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[1][1] > 0


def test_roles_mask(oracle, games):
    st, W, part, bad = games
    live = st[np.flatnonzero(part)[[0, 3, 6, 13, 14]]]
    roles = live[:, cs.F_META, cs.M_ROLE]
    assert set(roles.tolist()) == {0, 1, 2}
    full = phr.playouts_hidden(oracle, live, 2, seed=3)
    lord = phr.playouts_hidden(oracle, live, 2, seed=3, roles=0b010)
    assert np.array_equal(lord[0][roles == 1], full[0][roles == 1]) and not lord[0][roles != 1].any()
    assert 0 < lord[1][1] < full[1][1]
    assert not phr.playouts_hidden(oracle, live, 2, seed=3, roles=0)[1].any()


# the pool {a, a, b, b, c} with n_next = 2: the next player's count vector (a, b, c) is multivariate hypergeometric
POOL_P = {(2, 0, 0): 1 / 10, (0, 2, 0): 1 / 10, (1, 1, 0): 4 / 10, (1, 0, 1): 2 / 10, (0, 1, 1): 2 / 10}
CHI2_BOUND = 23.513          # the 1 - 1e-4 quantile of chi-squared with 4 degrees of freedom (5 outcomes)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_uniformity(oracle, seed):
    assert abs(sum(POOL_P.values()) - 1) < 1e-12
    assert math.exp(-CHI2_BOUND / 2) * (1 + CHI2_BOUND / 2) <= 1e-4 < math.exp(-23.5 / 2) * (1 + 23.5 / 2)   # df = 4 in closed form
    n = 20000
    st = hc._table({0: 1}, {5: 1, 6: 1}, {5: 1, 6: 1, 7: 1}, role=1)
    W, part, bad = phr.worlds(oracle, st, n, seed=seed)
    assert part.all() and phr.decode(st)[0][2].tolist() == [0] * 5 + [2, 2, 1] + [0] * 7
    seen = {}
    for row in W[0, :, 0, 5:8]:
        seen[tuple(row.tolist())] = seen.get(tuple(row.tolist()), 0) + 1
    assert set(seen) <= set(POOL_P) and sum(seen.values()) == n
    chi2 = sum((seen.get(o, 0) - n * p) ** 2 / (n * p) for o, p in POOL_P.items())
    print(f"seed {seed}: chi2 = {chi2:.3f} (bound {CHI2_BOUND})")
    assert chi2 < CHI2_BOUND


def test_domain(oracle):
    names, st = hc.out_of_domain()
    assert cs.running(st).all()
    for i, name in enumerate(names):
        assert not phr.decode(st[i:i + 1])[0][5], name
    sentinel = np.full((len(st), 2, 2, 16), 0x5A, np.uint8)
    W, part, bad = phr.worlds(oracle, st, 2, out=sentinel.copy())
    assert bad.all() and not part.any() and np.array_equal(W, sentinel)
    wins, totals, bad = phr.playouts_hidden(oracle, st, 2)
    assert bad.all() and not wins.any() and not totals.any()
    # the state they are variants of is inside the domain
    base = hc._table({0: 2, 5: 1}, {3: 2, 6: 1}, {3: 1, 4: 2, 9: 1}, role=1)
    assert phr.decode(base)[0][5]


def test_degenerate_pools(oracle, table):
    names, st = hc.degenerate()
    cs.check_consistent(st, table)
    dec = phr.decode(st)
    sizes = [(d[3], d[4]) for d in dec]
    assert (1, 4) in sizes and (4, 1) in sizes and (1, 1) in sizes
    assert sum(d[2][13] == 1 and d[2][14] == 1 for d in dec) >= 3 and sum((d[2][:13] == 4).any() for d in dec) >= 2
    n = 64
    W, part, bad = phr.worlds(oracle, st, n, seed=5)
    assert part.all() and not bad.any()
    for t, d in enumerate(dec):
        assert np.array_equal(W[t, :, 0, :15].astype(int) + W[t, :, 1, :15], np.broadcast_to(d[2], (n, 15))), names[t]
        assert (W[t, :, 0, 15] == d[3]).all() and (W[t, :, 1, 15] == d[4]).all()
        assert len({W[t, k].tobytes() for k in range(n)}) > 1, names[t]    # more than one deal is possible, and is dealt
    wins, totals, _ = phr.playouts_hidden(oracle, st, 4, seed=5)
    assert totals[1] == 4 * pr.root_lists(oracle, st)[0].sum() and totals[2] == 0


def differing_worlds(got, want):
    """the (t, k) at which two world arrays differ: the comparison the GPU tests make is exact"""
    return [tuple(x) for x in np.argwhere((np.asarray(got) != np.asarray(want)).any((2, 3))).tolist()]


def test_perturbation_control(oracle, games):
    st, W, part, bad = games
    assert differing_worlds(W, W.copy()) == []
    t = int(np.flatnonzero(part)[4])
    # one card swapped between the two sampled hands of one world: sizes and conservation still hold
    P = W.copy()
    a = int(np.flatnonzero(P[t, 2, 0, :15] > 0)[0])
    b = int(np.flatnonzero((P[t, 2, 1, :15] > 0) & (np.arange(15) != a))[0])
    P[t, 2, 0, a] -= 1; P[t, 2, 1, a] += 1
    P[t, 2, 1, b] -= 1; P[t, 2, 0, b] += 1
    assert np.array_equal(P[t, 2, :, :15].sum(0), W[t, 2, :, :15].sum(0)) and np.array_equal(P[t, 2, :, :15].sum(1), W[t, 2, :, 15])
    assert differing_worlds(P, W) == [(t, 2)]
    # the keys drawn from domain 4 instead of 5
    D = phr.worlds(oracle, st, K, seed=hc.SEED, gid_base=hc.GID_BASE, domain=4)[0]
    diff = differing_worlds(D, W)
    assert len(diff) > 0.9 * part.sum() * K and {x[0] for x in diff} <= set(np.flatnonzero(part).tolist())


def test_plain_payload_to_playout_state(oracle, games):
    serving = importlib.import_module("doudizhu-rl_amd.serving")
    st = games[0]
    payloads = json.loads(json.dumps(serving.state_to_payloads(st)))
    assert all(set(p) == {"role_id", "cur_cards", "history", "left", "last_taken"} for p in payloads)
    back = serving.payloads_to_playout_state(payloads)
    assert np.array_equal(back[:, 3:10], st[:, 3:10])                      # histories, recent rows WITH category, taken
    assert np.array_equal(back[:, 0:3, 15], st[:, 0:3, 15])                # the three hand sizes
    for t in range(len(st)):
        role = int(st[t, cs.F_META, cs.M_ROLE])
        assert np.array_equal(back[t, role], st[t, role])
        assert not back[t, [(role + 1) % 3, (role + 2) % 3], :15].any()   # the opponents' cards are not in a payload
    run = cs.running(st)
    W = phr.worlds(oracle, back[run], K, seed=hc.SEED)[0]
    assert np.array_equal(W, phr.worlds(oracle, st[run], K, seed=hc.SEED)[0])


def test_hidden_symbols_exported():
    build = importlib.import_module("doudizhu-rl_amd.build")
    build.build()
    lib = importlib.import_module("doudizhu-rl_amd._lib")
    hdr = open(os.path.join(REPO, "include", "ddz_env.h")).read()
    declared = set(re.findall(r"\b(ddz_[a-z_0-9]+)\s*\(", hdr))
    assert {"ddz_playout_hidden", "ddz_playout_worlds"} <= declared
    assert "bit6" in hdr
    for jk in (False, True):
        L = lib.lib(jk=jk)
        assert L.ddz_abi_version() == 1
        for name in ("ddz_playout_hidden", "ddz_playout_worlds", "ddz_playout", "ddz_playout_choose"):
            assert hasattr(L, name) and name in lib.SYMBOLS
    L = lib.lib()
    assert L.ddz_playout_hidden(None, 1, 0, 1, 512, 7, None, None, None) == -2            # EHANDLE
    assert L.ddz_playout_worlds(None, 1, 0, 7, None, None) == -2
    assert L.ddz_playout(None, 1, 0, 1, 512, None, None, None) == -2                       # the open entry keeps its signature
