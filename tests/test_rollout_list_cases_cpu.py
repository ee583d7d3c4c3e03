"""The cases of tests/rollout_list_cases.py held to the CPU oracle, without a GPU: every case's list has the shape the case
declares (rows of the closed-form round, whether the kernel's scalar test asks the planner for a tail, whether the list really
goes on behind the round), and every forced draw was found -- so tests/test_gpu_rollout_list_cases.py cannot pass on cases
that never reach the seam between the round and the tail."""
import numpy as np
import pytest

import constructed_states as cs
import rollout_list_cases as rc

DENSE = 6144


@pytest.fixture(scope="module")
def table(oracle):
    return cs.Table(*oracle.action_table())


@pytest.fixture(scope="module")
def cases(oracle, table):
    return rc.build(oracle, table)


def _base_ids(lead):
    """the canonical ids a closed-form round can hold, the rocket apart"""
    return set(range(1, 55)) if lead else ({0} | set(range(42, 55)))


def _check_shapes(c, table):
    for k, name in enumerate(c.name):
        ids = c.ids[c.off[k]:c.off[k + 1]].tolist()
        assert ids == sorted(ids), name
        b = int(c.beat[k])
        n0, tail = rc.scalar_split(c.hand[k], int(table.cat[b]) if b else 0, int(table.value[b]), int(table.length[b]))
        assert (n0, tail) == (int(c.n0[k]), bool(c.tail[k])), (name, n0, tail)
        head, rest = ids[:n0], ids[n0:]
        base = _base_ids(b == 0)
        assert len(head) == n0 and all(i in base or (i == rc.ID_BIGBANG and not tail) for i in head), (name, ids)
        assert not any(i in base for i in rest), (name, ids)               # the round holds ALL of its ids
        assert bool(rest) == bool(c.more[k]), (name, ids)
        assert tail or not rest, (name, ids)                               # the scalar test is a superset of the truth
        if rest and not b:
            assert all(i > 54 for i in rest), name


def test_every_case_has_its_shape(cases, table):
    _check_shapes(cases, table)
    lead = cases.beat == 0
    # the kinds of ply the seam separates are all there: closed-form and hybrid, leads and follows, and the superset case
    for sel in (lead, ~lead):
        assert (sel & ~cases.tail).sum() >= 5 and (sel & cases.tail & cases.more).sum() >= 5 and (sel & cases.tail & ~cases.more).sum() >= 1
    assert set(table.cat[cases.beat[~lead]].tolist()) == set(range(4, 15))           # every category above a triple is followed
    assert cases.n.max() > 40 and cases.hand.sum(1).max() == 20                      # a long list: the 20-card lead
    hybrid_rocket = cases.tail & cases.more & (cases.hand[:, rc.BJ] + cases.hand[:, rc.CJ] == 2)
    assert (hybrid_rocket & lead).any() and (hybrid_rocket & ~lead).any()            # the rocket inside a tail


def test_joker_kicker_cases_have_their_shape(oracle):
    with oracle.variant(jk=True):
        t = cs.Table(*oracle.action_table())
        c = rc.build(oracle, t, both_jokers_only=True)
        _check_shapes(c, t)
    assert len(c.name) >= 12 and (c.ids >= 13527).sum() >= 2                          # the extra ids are in play


@pytest.mark.parametrize("total", [None, DENSE])
def test_every_forced_draw_is_found(oracle, cases, total):
    states, case, index, trials = rc.tables(cases, total)
    assert (trials > 0).all()
    assert len(states) == (total or len(case)) and set(case.tolist()) == set(range(len(cases.name)))
    # the oracle, stepped once, plays the wanted row on every table
    (run,), _ = cs.reference_run(oracle, states, 0, None, auto_reset=True, iters=1)
    want = cases.rows[cases.off[case] + index]
    assert np.array_equal(run["traj"][:, :16], want)
    assert np.array_equal(run["traj"][:, 28:32].copy().view("<u4")[:, 0], index)
    # every index of the short lists, and both sides of the seam of the long ones
    for k in np.flatnonzero(cases.n > 40):
        got = set(index[case == k].tolist())
        assert {0, int(cases.n0[k]) - 1, int(cases.n0[k]), int(cases.n[k]) - 1} <= got
