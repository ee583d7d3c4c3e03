"""The constructed states of tests/constructed_states.py and the CPU oracle held to each other, without a GPU: what
tests/test_gpu_constructed_states.py compares the kernels with must itself put every action id in play, and the step the
oracle's C applies must be the step rule of envi.py:38-43 as numpy states it.  Figures measured here are asserted as floors
and recorded in DESIGN.md 5."""
import numpy as np
import pytest

import constructed_states as cs

NA = 13527


@pytest.fixture(scope="module")
def table(oracle):
    return cs.Table(*oracle.action_table())


@pytest.fixture(scope="module")
def fam(oracle, table):
    return cs.families(oracle, table)


@pytest.fixture(scope="module")
def fam_jk(oracle):
    with oracle.variant(jk=True):
        t = cs.Table(*oracle.action_table())
        return t, cs.families(oracle, t, first_id=NA)


def test_table_equals_the_fixture(table, golden):
    g = golden("action_table.npz")
    assert table.n == NA and np.array_equal(table.rows, g["rows"]) and np.array_equal(table.cat, g["cat_range"])
    assert np.array_equal(table.lookup(g["rows"]), np.arange(NA)) and table.lookup(np.array([2, 1] + [0] * 13)) == -1


def test_philox_equals_the_oracle(oracle):
    rng = np.random.default_rng(1)
    w = rng.integers(0, 1 << 32, (300, 6), dtype=np.uint64)
    w[0], w[1], w[2, :4] = 0, 0xFFFFFFFF, 0xFFFFFFFF
    got = np.stack(cs.philox4x32_10(*w.T), 1)
    for i in range(len(w)):
        assert got[i].tolist() == oracle.philox(w[i, :4], w[i, 4:]).tolist()
    # the draw of STEP_RANDOM as the oracle makes it (oracle/ddz_oracle.c, ddzo_env_step), a table id beyond 2^32
    gid, ep, ply, n, seed = (1 << 40) + 5, 0xFFFFFFF0, 250, 497, (7 << 32) | 9
    x = oracle.philox([gid & 0xFFFFFFFF, gid >> 32, ep, (2 << 16) | ply], [seed & 0xFFFFFFFF, seed >> 32])[0]
    assert cs.random_index(gid, ep, ply, n, seed) == (int(x) * n) >> 32


def test_states_are_consistent(table, fam, fam_jk):
    for f in fam.values():
        cs.check_consistent(f.states, table)
    for f in fam_jk[1].values():
        cs.check_consistent(f.states, fam_jk[0])
    # ... and the check refuses what it promises to refuse
    s = fam["follow1"].states
    for field, byte in ((0, 3), (0, 15), (3, 0), (9, 14), (7, 15), (10, 2), (10, 6)):
        bad = s[:8].copy()
        bad[3, field, byte] ^= 1
        with pytest.raises(AssertionError):
            cs.check_consistent(bad, table)


def test_family_shapes(table, fam):
    """lead0: the lord, ply 0, 17 / 20 / 17; lead_exact: ply >= 3, the actor's turn, the hand IS the action, every recent row
    empty, everybody else holds a card; follow2: recent[role - 1] empty, recent[role + 1] the action."""
    s = fam["lead0"].states
    assert np.all(s[:, 10, 0] == 1) and not cs.meta_ply(s).any() and np.all(s[:, 0:3, 15] == [17, 20, 17]) and not s[:, 3:10].any()
    x = fam["exact"]
    role, t = x.states[:, 10, 0].astype(int), np.arange(x.T)
    assert np.all(cs.meta_ply(x.states) >= 3) and np.all((1 + cs.meta_ply(x.states)) % 3 == role) and not x.states[:, 6:9].any()
    assert np.array_equal(x.states[t, role, :15], table.rows[x.want]) and np.all(x.states[:, 0:3, 15] >= 1)
    assert np.all(x.states[:, 3:6, :15].sum(2) + x.states[:, 0:3, 15] == [17, 20, 17])
    for name, prev in (("follow1", 2), ("follow2", 1)):
        f = fam[name]
        role, t = f.states[:, 10, 0].astype(int), np.arange(f.T)
        assert np.array_equal(table.lookup(f.states[t, 6 + (role + prev) % 3, :15]), f.beat) and np.all(f.beat > 0)
        assert not f.states[t, 6 + (role + 3 - prev) % 3].any() and not f.states[t, 6 + role].any()
        assert np.array_equal(cs.to_beat(f.states, table), f.beat)
    e = fam["edges"].states
    idle = np.zeros(len(e), bool)
    idle[[cs.EDGE_FROZEN, cs.EDGE_UNDEALT]] = True
    assert np.array_equal(cs.running(e), ~idle) and e[cs.EDGE_FROZEN, 10, 1] == 1 and not e[cs.EDGE_UNDEALT].any()
    assert 0 < cs.EDGE_FROZEN < cs.EDGE_UNDEALT < len(e) - 1                          # between running tables
    assert np.all(cs.meta_episode(e[~idle]) == 0xFFFFFFF0) and set(cs.meta_ply(e[~idle])) == {250, 251, 252}
    assert np.all((1 + cs.meta_ply(e[~idle])) % 3 == e[~idle, 10, 0])


def test_every_id_is_legal_resolves_and_is_played(oracle, table, fam, fam_jk):
    """lead0 and lead_exact: the id is in its table's list, a forced episode exists within 65,536 trials (measured: 2,953 /
    2,809 at the most), and the oracle's STEP_RANDOM then plays exactly that id."""
    for tb, f in ((table, fam["lead0"]), (table, fam["exact"]), (fam_jk[0], fam_jk[1]["lead0"])):
        with oracle.variant(jk=tb.n > NA):
            assert f.legal.all(), "an id is not legal on its table: %s" % f.want[~f.legal][:5]
            assert (f.trials > 0).all(), "a forced pick did not resolve"
            assert np.all((f.trials >= 1) & (f.trials <= cs.MAX_TRIALS)) and f.trials.max() < 4096
            assert np.array_equal(f.ids[f.off[:-1] + f.index], f.want)
            (r,), _ = cs.reference_run(oracle, f.states, oracle.STEP_RANDOM, auto_reset=False)
            assert np.array_equal(r["traj"][:, :16], tb.row16[f.want]) and not r["traj"][:, 19].any()
            assert np.array_equal(r["traj"][:, 28:32].copy().view("<i4")[:, 0], f.index)
    assert fam["lead0"].n.sum() == 3257069 and fam["lead0"].n.max() == 497       # measured; 497 = the proven maximum
    assert fam["exact"].T == 34250


def test_every_id_is_applied_in_every_family_it_belongs_to(table, fam, fam_jk):
    assert np.array_equal(fam["lead0"].want, np.arange(1, NA))
    assert np.array_equal(fam_jk[1]["lead0"].want, np.arange(NA, NA + 24))
    x = fam["exact"]
    role = x.states[:, 10, 0]
    for r in range(3):
        ids = np.flatnonzero(table.cards <= cs.DEALT[r])[1:]
        assert np.array_equal(x.want[role == r], ids) and len(ids) == (10362, 13526, 10362)[r]
    # an action of all 20 cards ends the game: nobody ever faces it.  Every other id is faced, in both follow families
    faced = np.flatnonzero(table.cards < 20)[1:]
    assert len(faced) == 10373
    for name in ("follow1", "follow2"):
        assert np.array_equal(fam[name].beat, faced)
    assert fam_jk[1]["follow1"].T == 24 and fam_jk[1]["follow2"].T == 24


def test_every_category_and_length_is_faced(table, fam):
    """every (category, length) of the action table that fewer than 20 cards can form -- the three that take all 20
    (10 pairs in a row, 5 triples + 5 singles, 4 triples + 4 pairs) can only be a game's last action"""
    every = set(zip(table.cat[1:].tolist(), table.length[1:].tolist()))
    only20 = {(8, 10), (10, 5), (11, 4)}
    assert only20 <= every and all(np.all(table.cards[(table.cat == c) & (table.length == n)] == 20) for c, n in only20)
    for name in ("follow1", "follow2"):
        b = fam[name].beat
        assert set(zip(table.cat[b].tolist(), table.length[b].tolist())) == every - only20
    assert set(table.cards[fam["follow1"].beat]) == set(table.cards[1:]) - {20}


def test_follow_answers(table, fam):
    """follow1: the planted same-category answer is what the test plays; measured 7,176 of 10,373 tables (all the deck
    allows), 8,031 with any move but the pass; follow2 (random hands): 2,142 tables play a move, 357 of the category faced"""
    f = fam["follow1"]
    same = (table.cat[f.want] == table.cat[f.beat]) & (f.want > 0)
    assert same.sum() >= 7176 and (f.n > 1).sum() >= 8031
    assert set(table.cat[f.beat[same]]) == set(range(1, 15)) - {12}          # nothing beats the rocket
    g = fam["follow2"]
    assert (g.want > 0).sum() >= 2142 and ((table.cat[g.want] == table.cat[g.beat]) & (g.want > 0)).sum() >= 357


@pytest.mark.parametrize("name", ["lead0", "exact", "follow1", "follow2", "edges"])
def test_step_rule_in_numpy_equals_the_oracle(oracle, table, fam, name):
    """hand - action, history and taken + action, recent = the action, cards left (envi.py:38-43), stated in numpy: equal
    to the oracle's post-step state on every table -- the GPU comparison does not rest on the oracle's C alone"""
    f = fam[name]
    (r,), st = cs.reference_run(oracle, f.states, oracle.STEP_CHOICE, f.index, auto_reset=False)
    assert np.array_equal(cs.step(f.states, table, np.maximum(f.want, 0)).reshape(-1), r["state"])
    assert not r["illegal"][f.index >= 0].any() and st["plies"] == (f.index >= 0).sum()
    if name == "lead0":
        assert st == {"plies": 13526, "episodes": 3153, "lord_wins": 3153, "up_wins": 0, "down_wins": 0}
    if name == "exact":
        assert st["episodes"] == f.T and (st["up_wins"], st["lord_wins"], st["down_wins"]) == (10362, 13526, 10362)


def test_lead_comes_back_after_two_passes(oracle, table, fam):
    """three iterations from lead0 (the 3-iteration rollout launch): the tables on which both farmers pass behind a forced
    action of 6 or more cards, so that the lord leads again -- measured 3,096"""
    assert lead_back(cs.reference_run(oracle, fam["lead0"].states, iters=3)[0], table, fam["lead0"].want) >= 3096


def lead_back(run, table, want):
    passed = [(~r["traj"][:, :15].any(1)) & (r["traj"][:, 19] == 0) for r in run]
    assert np.array_equal(table.lookup(run[0]["traj"][:, :15]), want)
    return int((passed[1] & passed[2] & (run[0]["traj"][:, 17] == 0) & (table.cards[want] >= 6)).sum())


def test_the_comparison_rejects_a_perturbed_result(oracle, table, fam):
    f = fam["follow1"]
    (want,), _ = cs.reference_run(oracle, f.states, oracle.STEP_CHOICE, f.index)
    assert cs.differences({k: v.copy() for k, v in want.items()}, want) == []
    st = want["state"].reshape(-1, 11, 16)
    t = int(np.flatnonzero(f.n > 2)[0])

    def off_by_one_nibble(g):
        g["state"].reshape(-1, 11, 16)[5, 0, 3] += 1

    def wrong_category(g):
        g["state"].reshape(-1, 11, 16)[t, 6 + (st[t, 10, 0] + 2) % 3, 15] ^= 1

    def neighbouring_index(g):
        g["traj"][t, 28] += 1

    def swapped_rows(g):
        o = g["off"][t]
        g["rows"][[o, o + 1]] = g["rows"][[o + 1, o]]
        g["ids"][[o, o + 1]] = g["ids"][[o + 1, o]]

    for p in (off_by_one_nibble, wrong_category, neighbouring_index, swapped_rows):
        g = {k: v.copy() for k, v in want.items()}
        p(g)
        assert cs.differences(g, want), p.__name__
