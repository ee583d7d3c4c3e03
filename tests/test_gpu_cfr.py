"""GPU (-m gpu): ddz_cfr / ddz_cfr_choose against CFR spec v1 restated on the CPU oracle (tests/cfr_reference.py): n, ids,
sigma (as bit patterns), value (as bit patterns) and totals are compared EXACTLY, in both builds.  The batch is
cfr_cases.batch: at most 32 constructed tables; the restatement solves each table once per module for every iteration
count.  The coverage conditions are read from the restatement's own sizes and asserted."""
import importlib

import numpy as np
import pytest
import torch

import cfr_cases as cc
import cfr_reference as cr

pytestmark = pytest.mark.gpu
SEED, GID_BASE = 11, 2 ** 32 + 77


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(oracle, golden):
    rows = oracle.action_table()[0]
    states, names = cc.batch(oracle, rows, golden("cfr_reference.npz"), scramble=np.random.default_rng(3))
    return states, names


_refs = {}


def ref(oracle, states, iterations, **kw):
    k = (states.tobytes(), iterations, tuple(sorted(kw.items())))
    if k not in _refs:
        _refs[k] = cr.cfr(oracle, states, iterations, **kw)
    return _refs[k]


def _env(pkg, states, **kw):
    env = pkg.BatchedEnv(len(states), seed=SEED, device=_dev(), table_id_base=GID_BASE, **kw)
    env.state_import(torch.from_numpy(np.ascontiguousarray(states).reshape(-1)))
    return env


def _run(env, iterations, **kw):
    totals = torch.zeros(4, dtype=torch.int64, device=_dev())
    n, ids, sigma, value = env.cfr(iterations, totals=totals, **kw)
    torch.cuda.synchronize()
    return n.cpu().numpy(), ids.cpu().numpy(), sigma.cpu().numpy(), value.cpu().numpy(), totals.cpu().numpy()


def _same(got, want, rows=None):
    for name, g, w in zip(("n", "ids", "sigma", "value", "totals"), got, want[:5]):
        g, w = np.asarray(g), np.asarray(w)
        if rows is not None:
            if name == "totals":
                continue                                          # (the totals of a part of the batch: the caller's sum)
            g, w = g[rows], w[rows]
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)          # bit patterns
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:8].tolist())


@pytest.mark.parametrize("iterations", [0, 1, 2, 8])
def test_batch_exactly(pkg, oracle, cases, iterations):
    states, names = cases
    want = ref(oracle, states, iterations)
    env = _env(pkg, states)
    _same(_run(env, iterations), want)
    assert env.status() == want[5] == cr.STATUS_DOMAIN
    n = want[0]
    assert (n > 0).sum() == 22 and (n == 0).sum() == 2 and (n == -1).sum() == 4
    if iterations == 0:
        k = n[0]
        assert (want[2][0, :k] == 1.0 / k).all() and (want[3] == 0).all()


def test_taken_above_the_deck(pkg, oracle):
    """a rank taken more often than the deck holds it, the pool's size still right: n = -1 and status bit 6 from the
    per-rank test alone (the domain test k_cfr shares with the hidden-hand playouts and search)"""
    states = cc.taken_above_deck(oracle, oracle.action_table()[0])
    want = cr.cfr(oracle, states, 2)
    assert want[0][0] > 0 and want[0][1] == -1 and want[5] == cr.STATUS_DOMAIN
    env = _env(pkg, states)
    _same(_run(env, 2), want)
    assert env.status() == cr.STATUS_DOMAIN


def test_coverage(oracle, cases):
    """what the batch makes the kernel walk through (the restatement's sizes; nothing runs on the device here)"""
    states, names = cases
    res = [r for r in ref(oracle, states, 8)[6] if r.n > 0]
    assert max(r.deals for r in res) == cr.MAX_DEALS == 90                   # the 90-deal case
    assert max(r.nodes for r in res) == 10512                               # the largest forest the sweep found
    assert max(r.widest for r in res) > 64                                  # a level wider than a wavefront: the lane loop wraps
    assert max(r.members for r in res) > 8                                  # an information set with more than 8 members
    assert max(r.probe_info for r in res) >= 2 and max(r.probe_hist for r in res) >= 2   # probe chains beyond one step
    assert max(r.n for r in res) == 5 and min(r.n for r in res) == 1
    assert max(r.depth for r in res) >= 10 and max(r.infosets for r in res) > 2048
    role = states[:, cr.F_META, cr.M_ROLE]
    assert {int(x) for x in role[:22]} == {0, 1, 2}


def test_joker_kicker_build(pkg, oracle, cases):
    """the second build of the same source: no endgame holds a joker-kicker row, the results are the same numbers"""
    states, _ = cases
    env = _env(pkg, states, native_joker_kickers=True)
    assert env.native_joker_kickers
    for iterations in (1, 8):
        with oracle.variant(jk=True):
            want = cr.cfr(oracle, states, iterations)
        _same(_run(env, iterations), want)
        _same(want, ref(oracle, states, iterations))
    assert env.status() == cr.STATUS_DOMAIN


@pytest.mark.parametrize("slots", ["fewer", "equal", "more"])
def test_slots_and_order(pkg, oracle, cases, slots):
    """the batch permuted, with fewer, exactly as many and more slots than tables inside the domain"""
    states, _ = cases
    perm = np.random.default_rng(5).permutation(len(states))
    st = np.ascontiguousarray(states[perm])
    want = ref(oracle, st, 2)
    inside = int((want[0] > 0).sum())
    k = {"fewer": 9, "equal": inside, "more": inside + 7}[slots]
    env = _env(pkg, st)
    got = _run(env, 2, slots=k)
    lost = got[0] == -2
    assert lost.sum() == max(0, inside - k) and (want[0][lost] > 0).all()
    _same(got, want, rows=~lost)
    assert (got[1][lost] == -1).all() and (got[2][lost] == 0).all() and (got[3][lost] == 0).all()
    res = want[6]
    kept = [res[t] for t in np.flatnonzero(~lost) if res[t].n > 0]
    assert got[4].tolist() == [sum(getattr(r, f) for r in kept) for f in ("deals", "nodes", "infosets", "pairs")]
    assert env.status() == cr.STATUS_DOMAIN | (cr.STATUS_CAPACITY if lost.any() else 0)


def test_opponents_count_bytes_and_rerun(pkg, oracle, golden, cases):
    states, _ = cases
    rows = oracle.action_table()[0]
    other, _ = cc.batch(oracle, rows, golden("cfr_reference.npz"), scramble=np.random.default_rng(99))
    assert not np.array_equal(states, other)
    env = _env(pkg, states)
    first = _run(env, 8)
    again = _run(env, 8)                                  # the same workspace, dirty from the first run
    _same(again, first)
    _same(_run(_env(pkg, other), 8), first)
    blank = other.copy()
    for t in range(len(blank)):
        role = int(blank[t, cr.F_META, cr.M_ROLE])
        for r in range(3):
            if r != role:
                blank[t, r, :15] = 0
    _same(_run(_env(pkg, blank), 8), first)


def test_env_is_only_read_and_roles(pkg, oracle, cases):
    states, _ = cases
    env = _env(pkg, states)
    env.legal_slab()
    before = [x.clone() for x in (env.state, env.counts, env.rows, env.ids)]
    want = ref(oracle, states, 1, roles=0b101)
    _same(_run(env, 1, roles=0b101), want)
    assert all(torch.equal(x, y) for x, y in zip(before, (env.state, env.counts, env.rows, env.ids)))
    role = states[:, cr.F_META, cr.M_ROLE]
    assert (want[0][role == 1] == 0).all() and (want[0][role != 1] != 0).sum() >= 10


def test_graph_capture(pkg, oracle, cases):
    states, _ = cases
    env = _env(pkg, states)
    totals = torch.zeros(4, dtype=torch.int64, device=_dev())
    out = env.cfr(2, totals=totals)                       # (everything allocated)
    torch.cuda.synchronize()
    once = totals.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            env.cfr(2, totals=totals, out=out)            # two launches in a row: no parallel branches
    torch.cuda.current_stream().wait_stream(s)
    want = ref(oracle, states, 2)
    for rep in (2, 3):
        out[0].fill_(7)
        out[2].fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        _same([x.cpu().numpy() for x in out], want[:4])
        assert torch.equal(totals, once * rep)


def test_choose(pkg, oracle, cases):
    states, _ = cases
    want = ref(oracle, states, 8)
    env = _env(pkg, states)
    solved = env.cfr(8)
    picks = set()
    for salt in range(12):
        got = env.cfr_choose(salt=salt, solved=solved).cpu().numpy()
        exp = cr.choose(oracle, want[0], want[1], want[2], seed=SEED, gid_base=GID_BASE, salt=salt)
        assert np.array_equal(got, exp), salt
        picks.add(tuple(got.tolist()))
    assert len(picks) > 1                                 # the salt moves the draw
    got = env.cfr_choose(greedy=True, solved=solved).cpu().numpy()
    assert np.array_equal(got, cr.choose(oracle, want[0], want[1], want[2], greedy=True))
    assert np.array_equal(got < 0, want[0] <= 0)
    own = env.cfr_choose(8, greedy=True).cpu().numpy()   # solve and choose in one call
    assert np.array_equal(own, got)
    env.legal_slab()
    done, r, illegal = env.step_slab(torch.from_numpy(np.where(got < 0, 0, got)).to(_dev()), pkg.STEP_IDS, auto_reset=False)
    assert not illegal.cpu().numpy()[want[0] > 0].any()   # the ids are moves of the tables' lists


def test_choose_on_constructed_buffers(pkg, oracle):
    T = 4
    env = pkg.BatchedEnv(T, seed=5, device=_dev(), table_id_base=2 ** 32 + 3)
    ids = np.array([[7, 9, 11] + [-1] * 13] * T, np.int32)
    sigma = np.zeros((T, 16))
    sigma[0, :3] = (0.25, 0.5, 0.25)
    sigma[1, :3] = (0.0, 1.0, 0.0)
    sigma[2, :3] = (1e-300, 0.0, 0.0)
    sigma[3, :3] = (0.4, 0.4, 0.2)
    n = np.array([3, 3, 3, 0], np.int32)
    solved = tuple(torch.from_numpy(x).to(_dev()) for x in (n, ids, sigma, np.zeros(T)))
    for salt in range(8):
        got = env.cfr_choose(salt=salt, solved=solved).cpu().numpy()
        assert np.array_equal(got, cr.choose(oracle, n, ids, sigma, seed=5, gid_base=2 ** 32 + 3, salt=salt))
    n[3] = 3
    solved = tuple(torch.from_numpy(x).to(_dev()) for x in (n, ids, sigma, np.zeros(T)))
    assert env.cfr_choose(greedy=True, solved=solved).cpu().tolist() == [9, 9, 7, 7]


def test_small_workspace_and_bad_arguments(pkg, cases):
    states, _ = cases
    env = _env(pkg, states)
    T = env.T
    n = torch.empty(T, dtype=torch.int32, device=_dev())
    ids = torch.empty((T, 16), dtype=torch.int32, device=_dev())
    sigma = torch.empty((T, 16), dtype=torch.float64, device=_dev())
    value = torch.empty(T, dtype=torch.float64, device=_dev())
    need = env.lib.ddz_cfr_work_bytes(2)
    assert need == 256 + 2 * 1728 * 1024 and env.lib.ddz_cfr_work_bytes(-1) == -1
    work = torch.empty(need, dtype=torch.uint8, device=_dev())
    args = lambda it, roles, slots, nbytes: (env._h, it, roles, slots, work.data_ptr(), nbytes, n.data_ptr(), ids.data_ptr(),
                                             sigma.data_ptr(), value.data_ptr(), None, None)
    assert env.lib.ddz_cfr(*args(8, 7, 2, need - 1)) == -4                 # DDZ_ECAP, from the host: nothing ran
    assert env.lib.ddz_cfr(*args(65, 7, 2, need)) == -1 and env.lib.ddz_cfr(*args(8, 8, 2, need)) == -1
    assert env.lib.ddz_cfr(*args(8, 7, 0, need)) == 0                      # no slot at all: every endgame reports -2
    torch.cuda.synchronize()
    got = n.cpu().numpy()
    assert (got == -2).sum() == 22 and (got == -1).sum() == 4 and env.status() == 64 | 128
    with pytest.raises(ValueError):
        env.cfr(65)


def test_serving_cfr_act_and_predictor_routing(pkg, oracle, cases):
    serving = importlib.import_module("doudizhu-rl_amd.serving")
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    states, _ = cases
    st = states[:22]
    payloads = serving.state_to_payloads(st)
    want = ref(oracle, st, 8)
    rows = oracle.action_table()[0]
    cards = lambda a: [int(x) for x in np.repeat(np.arange(3, 18), rows[a, :15].astype(int))]
    for greedy, salt in ((True, 0), (False, 4)):
        moves = serving.cfr_act(payloads, 8, device=_dev(), salt=salt, seed=SEED, greedy=greedy)
        exp = cr.choose(oracle, want[0], want[1], want[2], seed=SEED, gid_base=0, salt=salt, greedy=greedy)
        assert moves == [cards(a) for a in exp]
    with pytest.raises(ValueError):
        serving.cfr_act(serving.state_to_payloads(states[24:25]), 8, device=_dev())       # 7 cards: no endgame
    with pytest.raises(ValueError):
        serving.cfr_act(serving.state_to_payloads(states[26:27]), 8, device=_dev())       # rows that do not add up
    # the reference's switch at its thresholds (core.py:80, :88): 12 own cards -> Rule; 6 cards in all -> CFR; 7 -> RL1
    def payload(own, others, role=1):
        deck = [c for c in range(3, 16) for _ in range(4)] + [16, 17]
        mine, rest = deck[:own], deck[own:]
        left = {role: own, (role + 1) % 3: others[0], (role + 2) % 3: others[1]}
        hist = {r: [] for r in range(3)}
        hist[(role + 1) % 3] = rest[others[0] + others[1]:]
        return {"role_id": role, "cur_cards": mine, "history": hist, "left": left, "last_taken": {0: [], 1: [], 2: []}}
    batch = [payload(12, (5, 5)), payload(11, (5, 5)), payload(2, (2, 2)), payload(3, (2, 2)), payload(4, (1, 1), role=0),
             payload(13, (1, 1), role=2)]
    assert [serving.Predictor.route(p) for p in batch] == ["Rule", "RL1", "CFR", "RL1", "CFR", "Rule"]
    torch.manual_seed(0)
    nets = {r: glue.QNet(6).to(_dev()).eval() for r in range(3)}
    replies = serving.Predictor(nets, _dev(), seed=SEED).act(batch, greedy=True)
    assert [r["model"] for r in replies] == ["Rule", "RL1", "CFR", "RL1", "CFR", "Rule"]
    for p, r in zip(batch, replies):
        assert r["data"] and all(r["data"].count(c) <= p["cur_cards"].count(c) for c in r["data"])    # a lead from the hand
    assert [r["data"] for r in replies if r["model"] == "CFR"] == serving.cfr_act([batch[2], batch[4]], 8, device=_dev(),
                                                                                  seed=SEED, greedy=True)
