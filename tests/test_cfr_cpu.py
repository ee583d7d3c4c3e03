"""CPU: CFR spec v1 as tests/cfr_reference.py restates it, against the reference's own results
(tests/golden/cfr_reference.npz: server/CFR.py's deal() and initiate_game(), recorded by tests/golden/gen_cfr.py) and on
positions whose answer is known by hand.  The fixture records max_deviation = 0.0: the restatement's fixed deal order gave
the reference's numbers bit for bit on every recorded case."""
import numpy as np
import pytest

import cfr_cases as cc
import cfr_reference as cr


@pytest.fixture(scope="module")
def rows(oracle):
    return oracle.action_table()[0]


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("cfr_reference.npz")


@pytest.fixture(scope="module")
def solved(oracle, rows, fixture):
    """every case of the fixture, solved once"""
    return [cr.solve(oracle, s, 8, rows) for s in cc.golden_states(oracle, rows, fixture)]


def test_reference_sigma_at_every_root_information_set(rows, fixture, solved):
    g = fixture
    assert len(g["sigma"]) >= 200 and len(g["names"]) >= 12 and float(g["max_deviation"]) <= 1e-12
    worst, seen = 0.0, set()
    for c, hand, action, p in zip(g["case"], g["hand"], g["action"], g["sigma"]):
        first = int(g["first"][c])
        ids, mine = solved[c].sigma_all[(first, tuple(int(x) for x in hand), ())]
        j = [k for k, a in enumerate(ids) if np.array_equal(rows[a, :15], action)]
        assert len(j) == 1, (str(g["names"][c]), hand, action)
        worst = max(worst, abs(mine[j[0]] - float(p)))
        seen.add((int(c), tuple(int(x) for x in hand)))
    assert worst <= 1e-12, worst
    # every root information set of the restatement is in the fixture: nothing is left out on either side
    for c, r in enumerate(solved):
        first = int(g["first"][c])
        roots = {k[1] for k in r.sigma_all if k[0] == first and k[2] == ()}
        assert roots == {h for (cc_, h) in seen if cc_ == c}, str(g["names"][c])


def test_fixture_covers_the_shapes(fixture, solved):
    g = fixture
    assert max(r.deals for r in solved) == 90 and max(r.nodes for r in solved) >= 5826
    assert set(int(x) for x in g["first"]) == {0, 1, 2}                       # all three movers
    follow = [(int(f), int(o)) for f, o, b in zip(g["first"], g["owner"], g["beat"]) if b.any()]
    assert any((f - o) % 3 == 1 for f, o in follow) and any((f - o) % 3 == 2 for f, o in follow)   # both follow forms
    pools = g["pool"]
    assert (pools == 2).any() and (pools == 3).any() and (pools == 4).any() and (pools[:, 13:] == 1).all(1).any()


def test_deal_order_and_count(fixture):
    g = fixture
    for c in range(len(g["names"])):
        want = g["deals"][g["deal_case"] == c]
        got = cr.deal([int(x) for x in g["sizes"][c]], [int(x) for x in g["pool"][c]])
        assert len(got) == int(g["n_deals"][c]) == len(want)
        assert np.array_equal(np.array(got, np.int8), want), str(g["names"][c])
        assert len(set(got)) == len(got)
    assert int(g["n_deals"].max()) == cr.MAX_DEALS


def test_sigma_is_a_distribution(solved):
    for r in solved:
        for ids, s in r.sigma_all.values():
            assert len(ids) == len(s) <= cr.MAX_ACTIONS and min(s) >= 0.0
            assert abs(sum(s) - 1.0) <= 4 * np.finfo(np.float64).eps


def _state(rows, hand_cards, role, left, pool_cards, recent=None, fill=None):
    return cr.make_state(cc.vec(hand_cards), role, left, cr.DECK - np.array(cc.vec(pool_cards)), recent, rows, fill)


def test_hand_known_positions(oracle, rows):
    # a one-card lead: one move, played with certainty; the lord goes out at once in every deal
    r = cr.solve(oracle, _state(rows, [9], 1, [2, 1, 2], [4, 5, 9, 12, 13]), 8, rows)
    assert (r.n, r.ids, r.sigma, r.value) == (1, [1 + 6], [1.0], 1.0)
    # a forced win: the lord holds 3 and 2 against two farmers with one card each (4 and 5).  Leading the 3 loses to the
    # next farmer's card, leading the 2 wins (nobody beats it, then the 3 goes out): sigma concentrates on the 2
    r = cr.solve(oracle, _state(rows, [3, 15], 1, [1, 2, 1], [3, 4, 5, 15]), 8, rows)
    assert (r.n, r.ids, r.sigma) == (2, [1, 13], [0.0, 1.0])
    assert r.snap[0][0] == [0.5, 0.5] and r.snap[1][0] == [0.0, 1.0]
    # a forced pass: down faces the lord's 2 with a 5 and a 7
    two = oracle.lookup(np.array(cc.vec([15]), np.int8))
    r = cr.solve(oracle, _state(rows, [5, 7], 2, [1, 1, 2], [5, 7, 9, 11], {1: two}), 8, rows)
    assert (r.n, r.ids, r.sigma) == (1, [0], [1.0])


def test_opponents_count_bytes_are_not_read(oracle, rows, fixture):
    rng = np.random.default_rng(7)
    plain = cc.golden_states(oracle, rows, fixture)[2:9]
    noisy = cc.golden_states(oracle, rows, fixture, scramble=rng)[2:9]
    assert not np.array_equal(plain, noisy)
    a, b = cr.cfr(oracle, plain, 8), cr.cfr(oracle, noisy, 8)
    for x, y in zip(a[:6], b[:6]):
        assert np.array_equal(x, y)


def test_domain_edges(oracle, rows, fixture):
    states, names = cc.batch(oracle, rows, fixture)
    n, ids, sigma, value, totals, status, res = cr.cfr(oracle, states, 1)
    at = {nm: t for t, nm in enumerate(names)}
    assert n[at["idle: done"]] == 0 and n[at["idle: not dealt"]] == 0
    assert n[at["outside: 7 cards"]] == -1 and res[at["outside: 7 cards"]].status == 0
    for nm in ("outside: a left of 0", "outside: pool and hands differ", "outside: a hand outside the pool"):
        assert n[at[nm]] == -1 and res[at[nm]].status == cr.STATUS_DOMAIN, nm
    assert status == cr.STATUS_DOMAIN and (n[:22] > 0).all()
    assert (ids[n <= 0] == -1).all() and (sigma[n <= 0] == 0).all()
    # exactly 6 cards is inside; the actor's own size is its hand row's, whatever its byte 15 says
    six = states[0].copy()
    six[cr.F_HAND0 + 1, 15] = 9
    assert cr.solve(oracle, six, 1, rows).n == n[0]
    # roles: a table whose actor is left out is idle; slots: the tables behind the last slot get -2 and bit 7
    part = cr.cfr(oracle, states, 1, roles=0b010)
    role = states[:, cr.F_META, cr.M_ROLE]
    assert (part[0][role != 1] == 0).all() and np.array_equal(part[0][role == 1], n[role == 1])
    few = cr.cfr(oracle, states, 1, slots=5)
    assert (few[0] == -2).sum() == (n > 0).sum() - 5 and few[5] & cr.STATUS_CAPACITY


def test_sampling_rule(oracle):
    ids = np.array([[7, 9, 11] + [-1] * 13] * 4, np.int32)
    sigma = np.zeros((4, 16))
    sigma[0, :3] = (0.25, 0.5, 0.25)
    sigma[1, :3] = (0.0, 1.0, 0.0)
    sigma[2, :3] = (1e-300, 0.0, 0.0)                    # u is (almost surely) not below the sum: the last positive entry
    sigma[3, :3] = (0.2, 0.2, 0.6)
    n = np.array([3, 3, 3, 0], np.int32)
    hits = set()
    for salt in range(24):
        got = cr.choose(oracle, n, ids, sigma, seed=5, gid_base=2 ** 32 + 3, salt=salt)
        u = cr.draw_u(oracle, 2 ** 32 + 3, 5, salt)
        assert 0.0 <= u < 1.0
        assert got[0] == (7 if u < 0.25 else 9 if u < 0.75 else 11)
        assert got[1] == 9 and got[2] == 7 and got[3] == -1
        hits.add(int(got[0]))
    assert hits == {7, 9, 11}
    greedy = cr.choose(oracle, n, ids, sigma, greedy=True)
    assert greedy.tolist() == [9, 9, 7, -1]
    sigma[0, :3] = (0.4, 0.4, 0.2)
    assert cr.choose(oracle, n, ids, sigma, greedy=True)[0] == 7     # the FIRST maximum
