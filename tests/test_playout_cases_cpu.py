"""CPU: the constructed roots of tests/playout_cases.py have the shape they are meant to have, the reference's trace
(tests/playout_reference.py, trace=True) shows that the playouts from them walk through every branch k_playout has, and the
trace changes nothing of what the reference returns.  tests/test_gpu_playout_cases.py holds the kernels to the same
references on the same roots."""
import numpy as np
import pytest

import constructed_states as cs
import playout_cases as pc
import playout_reference as pr
from test_playout_reference_cpu import hand_built


@pytest.fixture(scope="module")
def table(oracle):
    return cs.Table(*oracle.action_table())


@pytest.fixture(scope="module")
def plain(oracle, table):
    sets = pc.build(oracle, table)
    return sets, {n: pc.reference(oracle, s) for n, s in sets.items()}


@pytest.fixture(scope="module")
def jk(oracle):
    with oracle.variant(jk=True):
        table = cs.Table(*oracle.action_table())
        sets = pc.build(oracle, table, jk=True)
        return table, sets, {n: pc.reference(oracle, s) for n, s in sets.items()}


def _check_set(s, table):
    assert s.states.shape == (s.T, 11, 16) and s.states.dtype == np.uint8 and s.K in (1, 2)
    cs.check_consistent(s.states, table)
    assert cs.running(s.states).all()
    role, ply = s.states[:, cs.F_META, cs.M_ROLE].astype(np.int64), cs.meta_ply(s.states)
    assert np.array_equal((role + 2) % 3, ply % 3), "the lord moves at plies 0 mod 3, down 1, up 2"
    beat = cs.to_beat(s.states, table)
    before = table.lookup(s.states[np.arange(s.T), cs.F_RECENT0 + (role + 2) % 3, :15])
    for t in range(s.T):
        if s.kind[t].startswith("follow"):
            assert (table.cat[beat[t]], table.length[beat[t]]) == s.group[t], s.names[t]
            assert (before[t] > 0) == (s.kind[t] == "follow1"), s.names[t]      # follow2: the player before has passed
        elif s.kind[t] != "deal":
            assert beat[t] == 0 and not s.states[t, cs.F_RECENT0:cs.F_RECENT0 + 3].any(), s.names[t]


def test_every_case_is_what_it_is_meant_to_be(oracle, table, plain):
    sets, refs = plain
    for name, s in sets.items():
        if name != "outside":
            _check_set(s, table)
    roots = sets["roots"]
    g = pc.groups(table)
    assert len(g) == 34 and {c for c, _ in g} == set(pc.CATEGORIES)
    role = roots.states[:, cs.F_META, cs.M_ROLE]
    for kind in ("follow1", "follow2"):
        mine = [t for t in range(roots.T) if roots.kind[t] == kind]
        assert {roots.group[t] for t in mine} == set(g)
        assert set(role[mine].tolist()) == {0, 1, 2}
        for answer in ("answer", "none"):          # both forms, in every role, for every category
            have = {(roots.group[t][0], int(role[t])) for t in mine if roots.names[t].endswith(answer)}
            lone = {pc.BIGBANG} if answer == "answer" else set()
            assert {c for c, _ in have} == set(pc.CATEGORIES) - lone
            assert all({r for c, r in have if c == cat} == {0, 1, 2} for cat in set(pc.CATEGORIES) - lone), answer
    # the form without an answer in kind: the oracle's list is the pass, bombs and the rocket alone
    n, off, ids = pr.root_lists(oracle, roots.states)
    for t in range(roots.T):
        if roots.names[t].endswith("none"):
            cats = set(table.cat[ids[off[t]:off[t + 1]]].tolist())
            assert cats <= {pc.EMPTY, pc.QUADRIC, pc.BIGBANG} and ids[off[t]] == 0, roots.names[t]
            if roots.group[t][0] == pc.BIGBANG:
                assert n[t] == 1, "facing the rocket only the pass is legal"
    # both jokers held: on a follow with a tail (an answer in kind in front of the rocket), without one, on a lead without
    jokers = roots.states[np.arange(roots.T), cs.F_HAND0 + role.astype(np.int64), pc.BJ:pc.CJ + 1].all(1)
    for kind, end in (("follow1", "answer"), ("follow1", "none"), ("follow2", "answer"), ("follow2", "none"), ("lead rocket", "")):
        assert any(jokers[t] and roots.kind[t] == kind and roots.names[t].endswith(end) for t in range(roots.T)), (kind, end)
    # the long list, the ply edges
    n_long = pr.root_lists(oracle, sets["long"].states)[0]
    assert n_long[0] >= pc.LONG_MIN and sets["long"].K == 2
    assert sorted(set(cs.meta_ply(sets["ply"].states).tolist())) == sorted(pc.PLY_SMALL)
    assert cs.meta_ply(sets["deals"].states).tolist() == [d[3] for d in pc.DEALS]
    # outside the domain: running tables, the actor's hand empty; everything else as a consistent state has it
    out = sets["outside"]
    assert tuple(out.names) == pc.OUTSIDE and cs.running(out.states).all()
    r = out.states[:, cs.F_META, cs.M_ROLE].astype(np.int64)
    assert not out.states[np.arange(2), cs.F_HAND0 + r].any()
    assert cs.to_beat(out.states, table)[0] == 0 and table.cat[cs.to_beat(out.states, table)[1]] == pc.SINGLE
    with pytest.raises(AssertionError, match="done <=> an empty hand"):
        cs.check_consistent(out.states, table)
    assert not refs["outside"][0].any() and not refs["outside"][1].any()


def test_the_playouts_walk_every_branch(table, plain):
    sets, refs = plain
    for name, (wins, totals, tr) in refs.items():
        assert totals[2] == 0, name + ": a playout stopped unfinished"
        assert (tr.winner >= 0).all() and tr.moves.sum() == totals[0] == tr.moves_per_table.sum()
    cov = pc.coverage(table, sets, refs)
    assert len(cov) == 2 * 34 + 14 + 3 + 13 + 14 + 4
    missing = [k for k, v in cov.items() if v is None]
    assert not missing, "no case reaches: " + "; ".join(missing)
    # every ply case reaches the wrap, the deals cross theirs; the ply counter of a playout counts up modulo 2^16
    for name in ("ply", "deals"):
        tr = refs[name][2]
        st = tr.steps
        for t in range(sets[name].T):
            mine = st[tr.t[st["copy"]] == t]
            assert ((mine["ply"] == 0) & (mine["s"] > 0)).any(), sets[name].names[t] + ": no playout reaches the wrap"
        same = st["copy"][1:] == st["copy"][:-1]
        assert np.array_equal(st["ply"][1:][same], (st["ply"][:-1][same] + 1) & 0xFFFF)
    assert (refs["deals"][2].moves >= 66).any()


def test_joker_kicker_sets(jk):
    table, sets, refs = jk
    assert table.n == pc.NA_PLAIN + 24
    for name, s in sets.items():
        _check_set(s, table)
        assert refs[name][1][2] == 0
    assert {g for g in sets["roots"].group if g is not None} == set(pc.groups(table))
    lead = sets["jk leads"]
    role = lead.states[:, cs.F_META, cs.M_ROLE].astype(np.int64)
    for t in range(lead.T):                        # the actor, or the second player, holds both jokers with a quad or triples
        who = (role[t] + (1 if lead.names[t].endswith("second") else 0)) % 3
        h = lead.states[t, cs.F_HAND0 + who, :15]
        assert h[pc.BJ] and h[pc.CJ] and (h[:13] >= 3).any(), lead.names[t]
    # a joker-kicker row is picked at a root and at a non-root ply, in the constructed leads themselves
    cov = pc.jk_coverage(table, {"jk leads": lead}, refs)
    assert all(v is not None for v in cov.values()), cov
    assert all(v is not None for v in pc.jk_coverage(table, sets, refs).values())
    assert sets["jk deals"].T == 8


def test_trace_changes_nothing(oracle, table):
    states, _, moves = hand_built(table)
    ref = oracle.OracleEnv(4, seed=11)
    ref.reset()
    for _ in range(30):
        ref.legal()
        ref.step(oracle.STEP_RANDOM, auto_reset=False)
    game = ref.state.reshape(4, 11, 16).copy()
    for st, kw in ((states, dict(seed=7, gid_base=3)), (game, dict(seed=11)), (game, dict(seed=11, salt=1)),
                   (states[3:5], {})):
        a = pr.playouts(oracle, st, 3, **kw)
        b = pr.playouts(oracle, st, 3, trace=True, **kw)
        assert len(a) == 2 and len(b) == 3
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == b[0].dtype
        tr = b[2]
        n = pr.root_lists(oracle, st, kw.get("seed", 0), kw.get("gid_base", 0))[0]
        assert len(tr.t) == 3 * n.sum() == b[1][1] and tr.moves_per_table.sum() == b[1][0]
        recs = tr.records()
        assert [(r["t"], r["j"], r["k"]) for r in recs] == [(t, j, k) for t in range(len(n)) for j in range(n[t]) for k in range(3)]
        assert all(len(r["plies"]) == r["moves"] and r["plies"][0][2] == r["j"] for r in recs)
        won = np.zeros_like(b[0])
        root_role = st[:, 10, 0]
        for r in recs:
            won[r["t"], r["j"]] += r["winner"] >= 0 and (r["winner"] == 1) == (root_role[r["t"]] == 1)
        assert np.array_equal(won, b[0])
    tr = pr.playouts(oracle, states, 3, seed=7, gid_base=3, trace=True)[2]
    assert tr.moves_per_table.tolist() == [3 * m for m in moves] == [3, 9, 9, 0, 0, 3]
    # table 1: the lord follows a 3 with one pass since (id 1); pass or its 9 (id 7); after the pass down leads and wins
    assert tr.plies(3)[0][2:] == (0, 0, 1, False) and tr.plies(3)[1][4:] == (0, True)
    assert tr.plies(6)[0][2:] == (1, 7, 1, False) and tr.winner[6] == 1 and tr.winner[3] == 2


def test_first_max_ids_on_the_choose_patterns():
    stride = pr.STRIDE
    names = set()
    for T in (1, 6, 9):
        seen = set()
        for name, counts, ids, wins, want, first in pc.choose_problems(T, stride):
            live = np.clip(counts.astype(np.int64), 0, stride)
            got = pr.first_max_ids(wins, live, np.arange(T + 1) * stride, ids.reshape(-1))
            assert np.array_equal(got, want), name
            assert np.array_equal(want, np.where(first >= 0, 1000 * np.arange(T) + first, -1)), name     # the closed form
            assert np.array_equal(want < 0, counts <= 0)
            seen |= {(name, int(c)) for c in counts}
            names.add(name)
        assert seen == {(n, c) for n in names for c in pc.COUNTS}
    assert len(names) == 8
