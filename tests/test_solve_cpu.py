"""CPU: solve spec v1 as tests/solve_reference.py restates it -- spec() against exact() on the constructed cases
(tests/solve_cases.py) and on the rollout positions the solver was sized on, the independence of proven values from chunks and
tt_entries, the coverage conditions of the case list read from spec()'s trace, the hidden form against open solves of its
worlds, choose(), engine.py's argument checks on a stand-in library, and the ABI's declarations."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import playout_hidden_reference as phr
import solve_cases as sc
import solve_reference as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ddz_solve_work_bytes", "ddz_solve", "ddz_solve_choose")


@pytest.fixture(scope="module")
def cases(oracle):
    return sc.batch(oracle)


@pytest.fixture(scope="module")
def solved(oracle, cases):
    """spec() at the defaults with its trace, and exact(), on the cases"""
    return sr.spec(oracle, cases[0], trace=True), sr.exact(oracle, cases[0])


def proven_equal(got, want_wins):
    n, wins, unknown = got[:3]
    for t in np.flatnonzero(n > 0):
        ok = unknown[t, :n[t]] == 0
        assert np.array_equal(wins[t, :n[t]][ok], want_wins[t, :n[t]][ok]), t
        assert not wins[t, :n[t]][~ok].any(), t


def test_hand_checked_cases(cases, solved):
    states, names, expected = cases
    (n, wins, unknown, totals, status, _), _ = solved
    assert status == 0 and not unknown.any()
    for t, e in enumerate(expected):
        if e is not None:
            assert n[t] == len(e) and list(wins[t, :n[t]]) == e, names[t]
    by_name = dict(zip(names, n))
    assert by_name["idle: done"] == 0 and by_name["idle: not dealt"] == 0 and by_name["outside: 13 cards"] == -1
    assert not wins[n <= 0].any() and not unknown[n <= 0].any()
    assert totals[2] == n[n > 0].sum() and totals[3] == 0
    assert {int(s[sc.F_META, sc.M_ROLE]) for s, k in zip(states, n) if k > 0} == {0, 1, 2}          # all three actors


def test_spec_agrees_with_exact_on_the_cases(solved):
    (n, wins, unknown, _, _, _), (ne, we) = solved
    assert np.array_equal(n[n > 0], ne[n > 0])
    assert not unknown.any()
    assert np.array_equal(wins, np.where((n > 0)[:, None], we, 0))


@pytest.mark.parametrize("max_cards,count", [(9, 32), (12, 44)])
def test_spec_agrees_with_exact_on_the_rollout_positions(oracle, max_cards, count):
    P = sc.rollout_positions(oracle, max_cards)
    assert len(P) == count
    n, wins, unknown, totals, status, tr = sr.spec(oracle, P, budget=65536, max_cards=max_cards, tt_entries=4096, trace=True)
    ne, we = sr.exact(oracle, P)
    assert status == 0 and (n > 0).all() and np.array_equal(n, ne)
    assert not unknown.any() and totals[3] == 0                      # none unknown at the default budget and table ...
    assert max(tr.nodes.values()) * 8 <= 65536                       # ... with a margin of 8x
    assert np.array_equal(wins, we)
    assert totals[0] == sum(tr.nodes.values()) and totals[1] == tr.hits and totals[2] == n.sum()


@pytest.mark.parametrize("chunks,tt_entries", [(1, 16), (1, 64), (3, 16), (3, 64), (3, 4096)])
def test_proven_values_do_not_depend_on_chunks_or_the_table(oracle, cases, solved, chunks, tt_entries):
    for states, max_cards in ((cases[0], 12), (sc.rollout_positions(oracle, 9), 9)):
        got = sr.spec(oracle, states, max_cards=max_cards, chunks=chunks, tt_entries=tt_entries)
        _, we = sr.exact(oracle, states)
        proven_equal(got, we)
        assert got[2].sum() <= 1                                      # (one move of one case outruns a table of 16 entries)


def test_proven_values_of_the_larger_positions_with_a_small_table(oracle):
    P = sc.rollout_positions(oracle, 12)
    got = sr.spec(oracle, P, chunks=3, tt_entries=64)
    proven_equal(got, sr.exact(oracle, P)[1])


def test_a_small_budget_leaves_moves_unknown(oracle, cases, solved):
    got = sr.spec(oracle, cases[0], budget=40)
    n, wins, unknown, totals, status = got
    assert status == 0 and unknown.any() and totals[3] == unknown.sum() and totals[2] + totals[3] == n[n > 0].sum()
    assert unknown.max() == 1 and not (wins & unknown).any()
    proven_equal(got, solved[1][1])
    assert np.array_equal(n, solved[0][0])
    one = sr.spec(oracle, cases[0], budget=1)          # one node: the position behind the root move, nothing below it
    assert one[3][0] <= one[0][one[0] > 0].sum()


def test_coverage_of_the_case_list(oracle, cases, solved):
    tr = solved[0][5]
    assert tr.leads == set(range(1, 15))                                             # every kind led
    assert {b for b, _ in tr.follows} == set(range(1, 15))                           # every kind to be beaten ...
    assert {(c, c) for c in range(1, 15) if c != 12} <= tr.follows                   # ... and answered in kind (but the rocket)
    assert {(c, 0) for c in range(1, 15)} <= tr.follows and (4, 12) in tr.follows and (13, 4) in tr.follows
    assert {7, 10, 11} <= tr.tail_lead and {5, 6, 10, 11, 13, 14} <= tr.tail_follow  # planner tails, led and followed
    assert tr.lead_backs > 0 and tr.root_lead_backs > 0                              # two passes, inside and at the root
    assert tr.transpositions > 0 and tr.farmer_for_partner > 0 and tr.depth < sr.MAX_DEPTH
    t = cases[1].index("more positions than a table of 16 holds")
    t16 = sr.spec(oracle, cases[0][t:t + 1], tt_entries=16, trace=True)[5]
    assert t16.replaced > 0                                                          # replacement in a table of 16 entries
    assert sum(t16.nodes.values()) > sum(v for (tt, _, _), v in tr.nodes.items() if tt == t) > 16


def test_hidden_form(oracle, cases):
    states = cases[0]
    K, salt, seed = 4, 5, 11
    rng = np.random.default_rng(3)
    n, wins, unknown, totals, status = sr.spec(oracle, states, worlds=K, hidden=True, salt=salt, seed=seed)
    noisy = sr.spec(oracle, sc.scrambled(states, rng), worlds=K, hidden=True, salt=salt, seed=seed)
    for a, b in zip((n, wins, unknown, totals, status), noisy):
        assert np.array_equal(a, b)                               # the opponents' count bytes are not read
    t_short = cases[1].index("outside the hidden form: pool and hands differ")
    assert status == sr.STATUS_DOMAIN and n[t_short] == -1 and n[cases[1].index("outside: 13 cards")] == -1
    W, part, bad = phr.worlds(oracle, states, K, seed, 0, salt)
    assert bad[t_short]
    total = np.zeros_like(wins)
    for k in range(K):
        world = np.stack([phr.with_world(s, W[t, k]) if part[t] else s for t, s in enumerate(states)])
        nk, wk, uk, _, _ = sr.spec(oracle, world)
        assert not uk.any()
        solved = (n > 0)
        assert np.array_equal(nk[solved], n[solved])              # the root list is the same in every world
        total += np.where(solved[:, None], wk, 0)
    assert np.array_equal(total, wins) and not unknown.any() and 0 < wins.max() <= K
    lord = sr.spec(oracle, states, worlds=K, hidden=True, salt=salt, seed=seed, roles=0b010)
    is_lord = states[:, sc.F_META, sc.M_ROLE] == 1
    assert np.array_equal(lord[0], np.where(is_lord, n, 0)) and np.array_equal(lord[1], np.where(is_lord[:, None], wins, 0))


def test_choose():
    n = np.array([4, 3, 2, 0, -1, 3], np.int32)
    off = np.arange(6) * 8
    ids = np.arange(48, dtype=np.int32) + 100
    wins, unknown = np.zeros((6, 8), np.int32), np.zeros((6, 8), np.int32)
    wins[0, :4], unknown[0, :4] = [1, 2, 2, 0], [1, 1, 0, 0]     # most wins, then fewest unknown: index 2; not every world
    wins[1, :3], unknown[1, :3] = [0, 3, 3], [0, 0, 0]           # ties to the lowest index: 1; proven winning
    unknown[2, :2] = [1, 0]                                      # no win: the fewest unknown, index 1; not all proven
    wins[5, :3] = [0, 0, 0]                                      # every move proven losing
    choice, value = sr.choose(n, off, ids, wins, unknown, worlds=3)
    assert list(choice) == [102, 109, 117, -1, -1, 140] and list(value) == [-1, 1, -1, -1, -1, 0]


# ---- engine.py's argument checks, on a stand-in library (as tests/test_engine_arguments_cpu.py)
T, STRIDE = 4, 512
i32, i64, u8 = torch.int32, torch.int64, torch.uint8


class StandIn:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ddz_"):
            raise AttributeError(name)
        if name.endswith("_bytes"):
            return lambda *a: 64
        return lambda *a: self.calls.append(name) or 0


@pytest.fixture()
def env(monkeypatch):
    E = importlib.import_module("doudizhu-rl_amd.engine")
    lib = StandIn()
    monkeypatch.setattr(E, "_stream", lambda device: None)
    e = object.__new__(E.BatchedEnv)
    e.lib, e.device, e.T, e.cap, e._h = lib, torch.device("cpu"), T, T * STRIDE, None
    e.host_mirror = e.native_joker_kickers = False
    e.ids, e.counts = torch.zeros(T * STRIDE, dtype=i32), torch.zeros(T, dtype=i32)
    e._legal_fresh = e._slab_fresh = e._csr_fresh = True
    e._pp = {k: E._p(getattr(e, k)) for k in ("counts", "ids")}
    return e


def solve_out():
    return (torch.zeros(T, dtype=i32), torch.zeros(T * STRIDE, dtype=i32), torch.zeros(T * STRIDE, dtype=i32))


def test_engine_valid_calls_reach_the_library(env):
    n, wins, unknown = env.solve(out=solve_out(), totals=torch.zeros(4, dtype=i64))
    assert env.lib.calls == ["ddz_solve"] and wins.shape == (T, STRIDE) and unknown.shape == (T, STRIDE) and n.shape == (T,)
    env.solve(hidden=True, worlds=4, roles=0b010, chunks=3, tt_entries=16, budget=100, max_cards=20)
    ids, value = env.solve_choose(out=torch.zeros(T, dtype=i32), value=torch.zeros(T, dtype=i32))
    env.solve_choose(solved=(n, wins, unknown))
    assert env.lib.calls == ["ddz_solve", "ddz_solve", "ddz_solve", "ddz_solve_choose", "ddz_solve_choose"]


BAD = {"dtype": lambda x: x.to(i64 if x.dtype == i32 else i32), "strided": lambda x: x.new_zeros(2 * x.numel())[::2],
       "short": lambda x: x.reshape(-1)[:-1].clone(), "over": lambda x: torch.cat((x.reshape(-1), x.reshape(-1)[:1])),
       "device": lambda x: torch.empty(x.shape, dtype=x.dtype, device="meta")}


@pytest.mark.parametrize("kind", BAD)
@pytest.mark.parametrize("which", ["out.0", "out.1", "out.2", "totals", "choose.out", "choose.value", "solved.1", "solved.2"])
def test_engine_refuses_one_bad_tensor(env, which, kind):
    if (which, kind) == ("totals", "over"):
        return                                          # totals: at least 4 elements
    name, _, k = which.partition(".")
    with pytest.raises(ValueError):
        if name == "out":
            out = list(solve_out())
            out[int(k)] = BAD[kind](out[int(k)])
            env.solve(out=tuple(out))
        elif name == "totals":
            env.solve(totals=BAD[kind](torch.zeros(4, dtype=i64)))
        elif name == "choose":
            env.solve_choose(solved=solve_out(), **{k: BAD[kind](torch.zeros(T, dtype=i32))})
        else:
            s = list(solve_out())
            s[int(k)] = BAD[kind](s[int(k)])
            env.solve_choose(solved=tuple(s))
    assert env.lib.calls == []


@pytest.mark.parametrize("args", [dict(budget=0), dict(budget=(1 << 30) + 1), dict(max_cards=0), dict(max_cards=21), dict(worlds=2),
                                  dict(worlds=0, hidden=True), dict(worlds=65537, hidden=True), dict(roles=0b010), dict(roles=8, hidden=True),
                                  dict(chunks=0), dict(chunks=65537), dict(tt_entries=0), dict(tt_entries=24), dict(tt_entries=1 << 21)])
def test_engine_refuses_bad_arguments(env, args):
    with pytest.raises(ValueError):
        env.solve(**args)
    with pytest.raises(ValueError):
        env.solve_choose(**args)
    assert env.lib.calls == []


def test_engine_needs_a_full_slab_and_ids(env):
    env.ids = None
    with pytest.raises(ValueError):
        env.solve_choose()
    env.cap = T * 64
    with pytest.raises(ValueError):
        env.solve()
    assert env.lib.calls == []


# ---- the ABI
def test_header_declares_the_solver():
    text = open(os.path.join(REPO, "include", "ddz_env.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b(int|int64_t) %s\(" % name, text), name
    assert re.search(r"#define DDZ_SOLVE_MAX_CARDS 20\b", text) and re.search(r"#define DDZ_SOLVE_MAX_DEPTH 60\b", text)
    lib = importlib.import_module("doudizhu-rl_amd._lib")
    assert all(name in lib.SYMBOLS for name in SYMBOLS)
    assert len(lib.SYMBOLS["ddz_solve"][1]) == 17 and len(lib.SYMBOLS["ddz_solve_choose"][1]) == 10


@pytest.mark.parametrize("jk", [False, True])
def test_library_exports_the_solver(jk):
    build = importlib.import_module("doudizhu-rl_amd.build")
    path = build.LIB_JK if jk else build.LIB
    if not os.path.exists(path) or build.stale(path):
        pytest.skip("the library has not been built on this machine")
    L = ctypes.CDLL(path)
    for name in SYMBOLS:
        assert hasattr(L, name), name
