"""CPU: tests/search_reference.py (search spec v1 (UCT) on the oracle) pinned on positions whose answer is known by hand and
on the invariants of a UCT tree, plus the exported symbols and the host-side argument checks of ddz_search.  The same
restatement is what tests/test_gpu_search.py holds ddz_search to."""
import importlib
import math
import os
import re

import numpy as np
import pytest

import constructed_states as cs
import playout_hidden_reference as phr
import playout_reference as pr
import search_reference as sr
from test_playout_reference_cpu import _position, hand_built

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHI2_BOUND = 23.513          # the 1 - 1e-4 quantile of chi-squared with 4 degrees of freedom (5 outcomes)


@pytest.fixture(scope="module")
def table(oracle):
    return cs.Table(*oracle.action_table())


def pair_of_threes():
    """the lord leads from {3, 3}; down holds a 4, up a 5: the pair ends the game, the single 3 wins only behind two passes"""
    return _position({1: {0: 2}, 2: {1: 1}, 0: {2: 1}}, role=1)


def farmer_root():
    """down (a farmer) leads; its partner up moves next: the two modes part at depth 1"""
    return _position({2: {0: 1, 1: 1, 4: 1}, 0: {2: 1, 5: 1, 7: 1}, 1: {3: 1, 6: 1, 8: 1}}, role=2)


def lord_root():
    return _position({1: {0: 1, 1: 1, 4: 1}, 2: {2: 1, 5: 1, 7: 1}, 0: {3: 1, 6: 1, 8: 1}}, role=1)


def mid_game(oracle, T=4, plies=36, seed=11):
    ref = oracle.OracleEnv(T, seed=seed)
    ref.reset()
    for _ in range(plies):
        ref.legal()
        ref.step(oracle.STEP_RANDOM, auto_reset=False)
    st = ref.state.reshape(T, 11, 16).copy()
    assert cs.running(st).all()
    return st


def test_value_is_five_single_roundings():
    v = sr.value(3, 7, 50, 0.7)
    assert v.dtype == np.float32
    ln = np.float32(math.log(50))
    want = np.float32(3) / np.float32(7) + np.float32(0.7) * np.sqrt((np.float32(2) * ln) / np.float32(7))
    assert v == want and sr.value(0, 1, 1, 0.7) == 0 and sr.value(2, 2, 9, 0.0) == 1
    assert sr.LN[1] == 0 and sr.LN[1000] == np.float32(math.log(1000)) and len(sr.LN) == sr.MAX_BUDGET + 1


def test_pair_of_threes_is_chosen(oracle, table):
    st = pair_of_threes()
    cs.check_consistent(st, table)
    n, off, ids = pr.root_lists(oracle, st)
    assert n.tolist() == [2]
    visits, wins, totals, items = sr.search(oracle, st, 40, seed=7, gid_base=3, trace=True)
    assert visits[0, :2].sum() == 40 and wins[0, 1] == visits[0, 1] > 0      # the terminal child wins every visit
    assert wins[0, 0] < visits[0, 0]
    choice = sr.choose(visits, wins, n, off, ids)
    assert table.rows[choice[0]][:15].tolist() == [2] + [0] * 14
    assert any(r["terminal"] for r in items[0].iters)                        # the terminal node was selected again
    assert totals[1] == 40 and totals[2] == 0 and totals[3] == len(items[0].nodes) - 1


def test_idle_tables_run_nothing(oracle, table):
    states, _, _ = hand_built(table)
    visits, wins, totals = sr.search(oracle, states[3:5], 5)
    assert not visits.any() and not wins.any() and not totals.any()


@pytest.mark.parametrize("mode", ("reference", "sides"))
def test_tree_invariants(oracle, mode):
    st = mid_game(oracle)
    budget, trees = 48, 2
    visits, wins, totals, items = sr.search(oracle, st, budget, trees=trees, mode=mode, seed=11, trace=True)
    assert visits.sum(1).tolist() == [budget * trees] * len(st)              # every iteration goes through one root child
    assert len(items) == len(st) * trees and totals[1] == budget * len(items) and totals[2] == 0
    assert (wins <= visits).all()
    for it in items:
        root = it.nodes[0]
        assert root.V == budget == sum(it.nodes[x].V for x in root.kids.values())
        assert len(it.iters) == budget and sum(r["expand"] is not None for r in it.iters) == len(it.nodes) - 1
        for nd in it.nodes[1:]:
            assert 0 <= nd.W <= nd.V and len(nd.kids) <= max(nd.n, 0)
            if not nd.terminal:
                assert nd.n > 0 and nd.V == 1 + sum(it.nodes[x].V for x in nd.kids.values())
            else:
                assert not nd.kids and nd.W in (0, nd.V)
    assert totals[0] == sum(r["moves"] for it in items for r in it.iters)
    # a tree does not depend on its neighbours: table 2 alone, at its own gid
    alone = sr.search(oracle, st[2:3], budget, trees=trees, mode=mode, seed=11, gid_base=2)
    assert np.array_equal(alone[0][0], visits[2]) and np.array_equal(alone[1][0], wins[2])


def test_budget_below_the_list_visits_each_child_once(oracle):
    st = mid_game(oracle, plies=3)
    n, _, _ = pr.root_lists(oracle, st)
    budget = int(n.min())
    assert budget >= 2
    visits, wins, totals = sr.search(oracle, st, budget, seed=11)
    assert visits.max() == 1 and visits.sum(1).tolist() == [budget] * len(st) and totals[3] == budget * len(st)


def test_first_expansion_index_is_uniform(oracle, table):
    st = _position({1: {0: 1, 1: 1, 2: 1, 3: 1, 5: 1}, 2: {6: 2}, 0: {7: 2}}, role=1)      # five singles, no line
    assert pr.root_lists(oracle, st)[0].tolist() == [5]
    T = 4000
    visits, _, _ = sr.search(oracle, np.repeat(st, T, 0), 1, seed=3, gid_base=2 ** 32 + 17)
    seen = visits[:, :5].sum(0)
    assert seen.sum() == T and (visits.sum(1) == 1).all()
    chi2 = float(((seen - T / 5) ** 2 / (T / 5)).sum())
    print(f"chi2 = {chi2:.3f} (bound {CHI2_BOUND})")
    assert chi2 < CHI2_BOUND


def test_modes(oracle, table):
    far, lord = farmer_root(), lord_root()
    cs.check_consistent(np.concatenate([far, lord]), table)
    a = sr.search(oracle, far, 60, mode="reference", seed=5, trace=True)
    b = sr.search(oracle, far, 60, mode="sides", seed=5, trace=True)
    assert any(not mx for r in a[3][0].iters for (_, _, _, mx, _, _) in r["sel"])          # the partner's node took a minimum
    assert all(mx for r in b[3][0].iters for (_, _, _, mx, _, _) in r["sel"])
    assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    # a lord root with a budget that never selects below the root: the root's own maximum is all there is
    n = int(pr.root_lists(oracle, lord)[0][0])
    budget = n + 2
    a = sr.search(oracle, lord, budget, mode="reference", seed=5, trace=True)
    b = sr.search(oracle, lord, budget, mode="sides", seed=5, trace=True)
    sels = [s for r in a[3][0].iters for s in r["sel"]]
    assert sels and all(depth == 0 and mx for (depth, _, _, mx, _, _) in sels)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_hidden_trees_play_on_the_worlds_of_spec_v2(oracle):
    st = mid_game(oracle, T=3, plies=20)
    trees = 3
    W, part, bad = phr.worlds(oracle, st, trees, seed=11, gid_base=5, salt=2, roles=0b111)
    assert part.all() and not bad.any()
    visits, wins, totals, items = sr.search(oracle, st, 6, trees=trees, seed=11, gid_base=5, salt=2, hidden=True, trace=True)
    assert len(items) == 3 * trees
    for it in items:
        role = int(st[it.t, cs.F_META, cs.M_ROLE])
        assert np.array_equal(it.root[(role + 1) % 3], W[it.t, it.c, 0]) and np.array_equal(it.root[(role + 2) % 3], W[it.t, it.c, 1])
        assert np.array_equal(it.root[role], st[it.t, role])
    # the opponents' count bytes are not read: emptied rows (sizes kept) give the same search
    blind = st.copy()
    for t in range(len(st)):
        role = int(st[t, cs.F_META, cs.M_ROLE])
        for r in ((role + 1) % 3, (role + 2) % 3):
            blind[t, r, :15] = 0
    again = sr.search(oracle, blind, 6, trees=trees, seed=11, gid_base=5, salt=2, hidden=True)
    assert np.array_equal(again[0], visits) and np.array_equal(again[1], wins) and np.array_equal(again[2], totals)
    # the roles mask leaves tables out
    role0 = int(st[0, cs.F_META, cs.M_ROLE])
    masked = sr.search(oracle, st, 6, trees=trees, seed=11, gid_base=5, salt=2, hidden=True, roles=0b111 ^ (1 << role0))
    assert not masked[0][0].any() and np.array_equal(masked[0][st[:, cs.F_META, cs.M_ROLE] != role0],
                                                      visits[st[:, cs.F_META, cs.M_ROLE] != role0])


def test_choose_compares_ratios_exactly():
    visits = np.array([[3, 0, 6, 2, 4]], np.int32)
    wins = np.array([[1, 0, 4, 1, 2]], np.int32)          # 1/3, -, 2/3, 1/2, 1/2
    ids = np.arange(10, 15, dtype=np.int32)
    off = np.array([0, 5])
    assert sr.choose(visits, wins, np.array([5]), off, ids).tolist() == [12]
    assert sr.choose(visits, wins, np.array([2]), off, ids).tolist() == [10]
    wins[0, 2] = 3                                         # 1/2 three times: the lowest index among them
    assert sr.choose(visits, wins, np.array([5]), off, ids).tolist() == [12]
    assert sr.choose(np.zeros_like(visits), wins, np.array([5]), off, ids).tolist() == [-1]


def test_search_symbols_exported_and_argument_checks():
    build = importlib.import_module("doudizhu-rl_amd.build")
    build.build()
    lib = importlib.import_module("doudizhu-rl_amd._lib")
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    hdr = open(os.path.join(REPO, "include", "ddz_env.h")).read()
    declared = set(re.findall(r"\b(ddz_[a-z_0-9]+)\s*\(", hdr))
    names = ("ddz_search", "ddz_search_choose", "ddz_search_work_bytes")
    assert set(names) <= declared
    assert int(re.search(r"#define DDZ_SEARCH_MAX_BUDGET (\d+)", hdr).group(1)) == sr.MAX_BUDGET
    assert int(re.search(r"#define DDZ_SEARCH_MAX_DEPTH (\d+)", hdr).group(1)) == sr.MAX_DEPTH
    assert hasattr(engine.BatchedEnv, "search") and hasattr(engine.BatchedEnv, "search_choose")
    for jk in (False, True):
        L = lib.lib(jk=jk)
        for name in names:
            assert hasattr(L, name) and name in lib.SYMBOLS
    L = lib.lib()
    assert L.ddz_search(None, 1, 1, 0, 0.7, 0, 0, 7, 512, None, None, None, None, 0, None) == -2            # EHANDLE
    assert L.ddz_search_choose(None, None, None, 512, None, None, None, None) == -2
    # the workspace is a function of the budget alone per tree: budget + 1 records of 24 bytes and 2^k >= 2 (budget + 1) slots
    per = {64: 1568 + 8 * 256, 1000: 24032 + 8 * 2048, 4096: 98336 + 8 * 16384}
    for budget, b in per.items():
        assert L.ddz_search_work_bytes(1, budget, 1) == b
        assert L.ddz_search_work_bytes(7, budget, 5) == 35 * b
    for bad in ((1, 0, 1), (1, 4097, 1), (1, 64, 0), (1, 64, 65537), (-1, 64, 1)):
        assert L.ddz_search_work_bytes(*bad) < 0
