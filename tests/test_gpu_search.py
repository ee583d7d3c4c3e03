"""GPU (-m gpu): ddz_search / ddz_search_choose against search spec v1 (UCT) restated on the CPU oracle
(tests/search_reference.py).  visits, wins and totals are compared EXACTLY.  Every reference is computed once per module
(cached by its arguments) and never written; the coverage conditions are read from the references' traces and asserted, so
the shapes cannot silently miss them."""
import importlib

import numpy as np
import pytest
import torch

import constructed_states as cs
import playout_cases as pc
import playout_hidden_cases as hc
import playout_reference as pr
import search_reference as sr

pytestmark = pytest.mark.gpu
SENTINEL = 0x3F3F3F3F
OUT_OF_DOMAIN = 64                                # status bit 6
GAMES = ((21, 0), (4, 2 ** 32 + 12345))       # (seed, table_id_base): the second puts the high half of gid into the counter
SMALL = 3                                     # the first SMALL hand-built tables are the endgames the 300-iteration trees grow on


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


def _pick(sets):
    """a handful of playout_cases' hand-built positions that suit a search: the three short rocket leads first (endgames:
    deep trees, terminal nodes met again), the follows with the fewest cards of either form, one exact lead, the longest
    lead list, the two tables outside the domain, one ply-counter wrap and one deal"""
    roots = sets["roots"]
    cards = roots.states[:, 0:3, 15].astype(np.int64).sum(1)
    rows = [t for t, k in enumerate(roots.kind) if k == "lead rocket"]
    for kind in ("follow1", "follow2"):
        ok = [t for t in np.argsort(cards, kind="stable") if roots.kind[t] == kind]
        rows += [x for x in ok if roots.names[x].endswith("answer")][:1] + [x for x in ok if roots.names[x].endswith("none")][:1]
    rows += [roots.names.index("lead exact category 8")]
    states = [roots.states[rows]]
    names = [roots.names[t] for t in rows]
    for name, take in (("long", 1), ("outside", 2), ("ply", 1), ("deals", 1)):
        states.append(sets[name].states[:take])
        names += sets[name].names[:take]
    return np.concatenate(states), names


@pytest.fixture(scope="module")
def plain(oracle):
    table = cs.Table(*oracle.action_table())
    states, names = _pick(pc.build(oracle, table))
    assert len(states) <= 16 and cs.running(states).all()
    return states, names


@pytest.fixture(scope="module")
def jk(oracle):
    with oracle.variant(jk=True):
        sets = pc.build(oracle, cs.Table(*oracle.action_table()), jk=True)
    return np.concatenate([sets["jk leads"].states[:6], sets["jk deals"].states[5:8]])


@pytest.fixture(scope="module")
def games(oracle):
    return {g: pc.deal_states(oracle, g[0], g[1], pc.PLIES8) for g in GAMES}


_refs = {}


def ref(oracle, key, states, budget, seed, gid_base, jk=False, **kw):
    """the reference of one call, computed once: (visits, wins, totals, items)"""
    k = (key, budget, seed, gid_base, jk, tuple(sorted(kw.items())))
    if k not in _refs:
        with oracle.variant(jk=jk):
            _refs[k] = sr.search(oracle, states, budget, seed=seed, gid_base=gid_base, trace=True, **kw)
    return _refs[k]


def _env(pkg, states, seed, gid_base, **kw):
    env = pkg.BatchedEnv(len(states), seed=seed, device=_dev(), table_id_base=gid_base, **kw)
    env.state_import(torch.from_numpy(np.ascontiguousarray(states).reshape(-1)))
    return env


def _run(env, budget, **kw):
    totals = torch.zeros(4, dtype=torch.int64, device=_dev())
    visits, wins = env.search(budget, totals=totals, **kw)
    return visits.cpu().numpy(), wins.cpu().numpy(), totals.cpu().numpy()


def _same(got, want):
    for name, g, w in zip(("visits", "wins", "totals"), got, want[:3]):
        assert np.array_equal(g, w), (name, np.argwhere(np.asarray(g) != np.asarray(w))[:8].tolist())


def _root_n(oracle, states):
    return pr.root_lists(oracle, states)[0]


def test_budgets_around_the_root_list(pkg, oracle, plain):
    """budgets 1, n - 1, n, n + 1 (n = the first table's list) and 64: before, at and behind the root's full expansion"""
    states, names = plain
    n_all = _root_n(oracle, states)
    n = int(n_all[0])
    assert n >= 3 and n_all.max() > 64 and (n_all[[names.index(x) for x in pc.OUTSIDE]] == 0).all()
    env = _env(pkg, states, pc.SEED, pc.GID_BASE)
    for budget in (1, n - 1, n, n + 1, 64):
        want = ref(oracle, "plain", states, budget, pc.SEED, pc.GID_BASE, trees=1)
        _same(_run(env, budget, trees=1), want)
        assert want[2][1] == budget * (len(states) - 2)           # the two tables outside the domain run nothing
    assert env.status() == 0


@pytest.mark.parametrize("trees,mode,c", [(2, "sides", 0.7), (5, "reference", 0.0), (2, "sides", 0.0), (5, "reference", 0.7)])
def test_trees_modes_and_c(pkg, oracle, plain, trees, mode, c):
    states, _ = plain
    want = ref(oracle, "plain", states, 64, pc.SEED, pc.GID_BASE, trees=trees, mode=mode, c=c)
    env = _env(pkg, states, pc.SEED, pc.GID_BASE)
    _same(_run(env, 64, trees=trees, mode=mode, c=c), want)
    assert want[0].sum() == 64 * trees * (len(states) - 2) and env.status() == 0


@pytest.mark.parametrize("mode", ["reference", "sides"])
def test_300_iterations(pkg, oracle, plain, mode):
    states = plain[0][:SMALL]
    want = ref(oracle, "small", states, 300, pc.SEED, pc.GID_BASE, trees=1, mode=mode)
    env = _env(pkg, states, pc.SEED, pc.GID_BASE)
    _same(_run(env, 300, trees=1, mode=mode), want)
    assert env.status() == 0


@pytest.mark.parametrize("game", GAMES)
def test_games_from_reset(pkg, oracle, games, game):
    st = games[game]
    env = _env(pkg, st, *game)
    assert env.legal_slab()[0].cpu().numpy()[0] > 55              # the lord's first lead: a list with planner tails
    for trees, mode in ((2, "reference"), (1, "sides")):
        want = ref(oracle, "games", st, 64, *game, trees=trees, mode=mode)
        assert want[2][2] == 0                                    # the reference's own result first: every playout finished
        _same(_run(env, 64, trees=trees, mode=mode), want)
    assert env.status() == 0


@pytest.mark.parametrize("trees,roles", [(1, 0b111), (3, 0b110)])
def test_hidden(pkg, oracle, games, trees, roles):
    st = games[GAMES[0]]
    want = ref(oracle, "games", st, 64, *GAMES[0], trees=trees, hidden=True, roles=roles, salt=3)
    env = _env(pkg, st, *GAMES[0])
    got = _run(env, 64, trees=trees, hidden=True, roles=roles, salt=3)
    _same(got, want)
    role = st[:, cs.F_META, cs.M_ROLE]
    part = ((roles >> role) & 1).astype(bool)
    assert part.any() and (got[0].sum(1) == np.where(part, 64 * trees, 0)).all() and env.status() == 0
    # the opponents' count bytes are never read
    blind = st.copy()
    for t in range(len(st)):
        for r in ((role[t] + 1) % 3, (role[t] + 2) % 3):
            blind[t, r, :15] = 0
    _same(_run(_env(pkg, blind, *GAMES[0]), 64, trees=trees, hidden=True, roles=roles, salt=3), want)


def _raw_hidden(pkg, env, budget, trees, salt):
    """ddz_search (hidden form) on visits / wins pre-filled with SENTINEL (BatchedEnv.search zeroes its own)"""
    env.legal_slab()
    n = env.T * env.slab_stride
    v = torch.full((n,), SENTINEL, dtype=torch.int32, device=_dev())
    w = torch.full((n,), SENTINEL, dtype=torch.int32, device=_dev())
    totals = torch.zeros(4, dtype=torch.int64, device=_dev())
    need = env.lib.ddz_search_work_bytes(env.T, budget, trees)
    work = torch.empty(need, dtype=torch.uint8, device=_dev())
    rc = env.lib.ddz_search(env._h, budget, trees, env.SEARCH_MODES["reference"], 0.7, salt, 1, 0b111, env.slab_stride,
                            v.data_ptr(), w.data_ptr(), totals.data_ptr(), work.data_ptr(), need, None)
    assert rc == 0
    torch.cuda.synchronize()
    return (v.view(env.T, -1).cpu().numpy().astype(np.int64), w.view(env.T, -1).cpu().numpy().astype(np.int64),
            totals.cpu().numpy())


def test_hidden_out_of_domain_between_running_tables(pkg, oracle):
    """k_search<true> on roots outside the hidden-hand domain (playout spec v2): status bit 6, nothing of theirs written,
    the tables between them searched as the reference searches them"""
    budget, trees, salt, seed, base = 8, 2, 3, 4, 2 ** 40
    names, bad = hc.out_of_domain()
    good = hc.degenerate()[1]
    st = np.zeros((2 * len(bad), 11, 16), np.uint8)
    st[0::2], st[1::2] = good[:len(bad)], bad
    want = sr.search(oracle, st, budget, trees=trees, seed=seed, gid_base=base, salt=salt, hidden=True)
    assert (want[0][0::2].sum(1) == budget * trees).all() and not want[0][1::2].any()   # the reference's own result first
    assert want[2][1] == budget * trees * len(bad)
    env = _env(pkg, st, seed, base)
    assert env.status() == 0
    v, w, tot = _raw_hidden(pkg, env, budget, trees, salt)
    assert env.status() & OUT_OF_DOMAIN
    assert (v[1::2] == SENTINEL).all() and (w[1::2] == SENTINEL).all(), "a table outside the domain was written"
    assert np.array_equal(v[0::2] - SENTINEL, want[0][0::2]) and np.array_equal(w[0::2] - SENTINEL, want[1][0::2])
    assert np.array_equal(tot, want[2])
    # one violation at a time: each raises the bit on its own, the table beside it is searched
    pair = sr.search(oracle, np.stack([good[0], bad[0]]), budget, trees=trees, seed=seed, salt=salt, hidden=True)
    for i, name in enumerate(names):
        one = _env(pkg, np.stack([good[0], bad[i]]), seed, 0)
        v, w, tot = _raw_hidden(pkg, one, budget, trees, salt)
        assert one.status() & OUT_OF_DOMAIN, name
        assert (v[1] == SENTINEL).all() and (w[1] == SENTINEL).all(), name
        assert np.array_equal(v[0] - SENTINEL, pair[0][0]) and np.array_equal(w[0] - SENTINEL, pair[1][0]), name
        assert np.array_equal(tot, pair[2]), name
    clean = _env(pkg, good, seed, 0)
    _raw_hidden(pkg, clean, budget, trees, salt)
    assert clean.status() == 0


def test_joker_kicker_build(pkg, oracle, jk):
    want = ref(oracle, "jk", jk, 64, pc.SEED, pc.GID_BASE, jk=True, trees=2)
    env = _env(pkg, jk, pc.SEED, pc.GID_BASE, native_joker_kickers=True)
    assert env.native_joker_kickers
    _same(_run(env, 64, trees=2), want)
    with oracle.variant(jk=True):
        ids = pr.root_lists(oracle, jk)[2]
    assert (ids >= pc.NA_PLAIN).any() and env.status() == 0       # joker-kicker rows are root moves of these trees


def test_coverage(oracle, plain, games):
    """what the references above walked through (their traces; nothing runs on the device here)"""
    states, names = plain
    items = []
    for trees, mode, c in ((2, "sides", 0.7), (5, "reference", 0.0), (5, "reference", 0.7)):
        items += ref(oracle, "plain", states, 64, pc.SEED, pc.GID_BASE, trees=trees, mode=mode, c=c)[3]
    big = [ref(oracle, "small", states[:SMALL], 300, pc.SEED, pc.GID_BASE, trees=1, mode=m)[3] for m in ("reference", "sides")]
    items += big[0] + big[1]
    items += ref(oracle, "games", games[GAMES[0]], 64, *GAMES[0], trees=2, mode="reference")[3]
    sels = [s for it in items for r in it.iters for s in r["sel"]]
    assert any(depth >= 2 for (depth, _, _, _, _, _) in sels)                                # selection at depth >= 2
    assert any(not mx for (_, _, _, mx, _, _) in sels)                                       # a minimum-branch selection
    assert any(tied and j == int(np.flatnonzero(v == v[j])[0]) for (_, _, j, _, tied, v) in sels)   # a tie broken by index
    assert any(r["terminal"] for it in items for r in it.iters)                              # a terminal node selected again
    assert any(it.nodes[0].n > 64 for it in items)                                           # a root list longer than 64 moves
    assert any(r["expand"] is not None and r["expand"][2] > 55 for it in items for r in it.iters)   # a list with a planner tail
    assert any(r["expand"] is not None and r["expand"][0] > 0 and r["expand"][2] > 30 for it in items for r in it.iters)
    assert max(it.probe.longest for it in big[0] + big[1]) >= 2                              # probe chains beyond one step
    assert max(len(it.nodes) for it in big[0] + big[1]) > 200


def test_env_is_only_read(pkg, games):
    st = games[GAMES[1]]
    env = _env(pkg, st, *GAMES[1])
    env.legal_slab()
    env.step_slab(mode=pkg.STEP_RANDOM, auto_reset=True)       # (some statistics to keep)
    stats = env.stats()
    before = [x.clone() for x in (env.state, env.counts, env.rows, env.ids, env.scratch)]
    env.search(20, trees=2, salt=9)
    env.search_choose(20, trees=1, hidden=True)
    torch.cuda.synchronize()
    after = (env.state, env.counts, env.rows, env.ids, env.scratch)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert env.stats() == stats and env.status() == 0


def test_salt_and_default_trees(pkg, games):
    st = games[GAMES[0]]
    env = _env(pkg, st, *GAMES[0])
    a, b, again = _run(env, 32, trees=1, salt=1), _run(env, 32, trees=1, salt=2), _run(env, 32, trees=1, salt=1)
    assert not np.array_equal(a[0], b[0])
    _same(again, a)
    v, w, tot = _run(env, 8)                                   # the default: trees enough to fill the device, at most 64
    assert tot[1] == 8 * 64 * len(st) and (v.sum(1) == 8 * 64).all() and (w <= v).all()


def test_search_choose(pkg, oracle, plain, games):
    for states, seed, base, kw in ((plain[0], pc.SEED, pc.GID_BASE, dict(trees=2, mode="sides", c=0.7)),
                                   (games[GAMES[0]], *GAMES[0], dict(trees=2, mode="reference"))):
        want = ref(oracle, "plain" if states is plain[0] else "games", states, 64, seed, base, **kw)
        n, off, ids = pr.root_lists(oracle, states)
        choice = sr.choose(want[0], want[1], n, off, ids)
        env = _env(pkg, states, seed, base)
        got = env.search_choose(64, **kw)
        assert np.array_equal(got.cpu().numpy(), choice)
        assert np.array_equal(choice < 0, n == 0)
        done, r, illegal = env.step_slab(got, pkg.STEP_IDS, auto_reset=False)   # (a table without a list is frozen)
        assert not illegal.any().item() and env.status() == 0


def test_choose_on_constructed_buffers(pkg):
    """ratios compared exactly in integers, ties to the lowest index, unvisited entries and entries beyond counts left out"""
    T, st = 3, 512
    env = pkg.BatchedEnv(T, seed=1, device=_dev())
    lib = importlib.import_module("doudizhu-rl_amd.engine")
    visits = np.zeros((T, st), np.int32)
    wins = np.zeros((T, st), np.int32)
    visits[0, [0, 70, 200]], wins[0, [0, 70, 200]] = (3, 6, 4), (2, 4, 1)            # 2/3 twice: index 0
    visits[1, [5, 130, 131]], wins[1, [5, 130, 131]] = (1000000, 3, 2000000), (999999, 3, 2000000)   # 1 at 130 first
    visits[2, 400], wins[2, 400] = 7, 7
    counts = torch.tensor([300, 200, 400], dtype=torch.int32, device=_dev())         # table 2: its only visit is beyond counts
    ids = torch.arange(T * st, dtype=torch.int32, device=_dev())
    out = torch.empty(T, dtype=torch.int32, device=_dev())
    v, w = torch.from_numpy(visits).to(_dev()), torch.from_numpy(wins).to(_dev())
    lib.check(env.lib.ddz_search_choose(env._h, counts.data_ptr(), ids.data_ptr(), st, v.data_ptr(), w.data_ptr(),
                                        out.data_ptr(), None))
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0, st + 130, -1]


def test_small_workspace_is_an_error(pkg, games):
    st = games[GAMES[0]]
    env = _env(pkg, st, *GAMES[0])
    env.legal_slab()
    n = env.T * env.slab_stride
    v = torch.zeros(n, dtype=torch.int32, device=_dev())
    w = torch.zeros(n, dtype=torch.int32, device=_dev())
    need = env.lib.ddz_search_work_bytes(env.T, 64, 2)
    work = torch.empty(need, dtype=torch.uint8, device=_dev())
    args = (env._h, 64, 2, 0, 0.7, 0, 0, 7, env.slab_stride, v.data_ptr(), w.data_ptr(), None, work.data_ptr())
    assert env.lib.ddz_search(*args, need - 1, None) == -4                            # DDZ_ECAP, from the host: nothing ran
    assert env.lib.ddz_search(*args, need, None) == 0
    torch.cuda.synchronize()
    assert v.view(env.T, -1).sum(1).cpu().tolist() == [128] * env.T and env.status() == 0


def test_graph_capture(pkg, oracle, games):
    st = games[GAMES[0]]
    env = _env(pkg, st, *GAMES[0])
    n = env.T * env.slab_stride
    bv = torch.empty(n, dtype=torch.int32, device=_dev())
    bw = torch.empty(n, dtype=torch.int32, device=_dev())
    totals = torch.zeros(4, dtype=torch.int64, device=_dev())
    kw = dict(trees=2, mode="reference", visits=bv, wins=bw, totals=totals)
    env.search(64, **kw)                                       # (everything allocated, the lists current)
    torch.cuda.synchronize()
    once = totals.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            env.search(64, **kw)                               # two memsets and one launch: no parallel branches
    torch.cuda.current_stream().wait_stream(s)
    want = ref(oracle, "games", st, 64, *GAMES[0], trees=2, mode="reference")
    for rep in (2, 3):
        bv.fill_(-1)
        bw.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bv.view(env.T, -1).cpu().numpy(), want[0]) and np.array_equal(bw.view(env.T, -1).cpu().numpy(), want[1])
        assert torch.equal(totals, once * rep)
    assert env.status() == 0


def test_serving_search_act(pkg, games):
    serving = importlib.import_module("doudizhu-rl_amd.serving")
    st = games[GAMES[0]][[0, 4, 7]]
    payloads = serving.state_to_full_payloads(st)
    rows = pkg.action_table(_dev()).cpu().numpy()
    for hidden in (False, True):
        moves = serving.search_act(payloads, 64, device=_dev(), salt=5, trees=3, hidden=hidden)
        imported = serving.payloads_to_playout_state(payloads) if hidden else serving.full_payloads_to_state(payloads)
        env = _env(pkg, imported, 0, 0)
        ids = env.search_choose(64, trees=3, salt=5, hidden=hidden).cpu().numpy()
        assert (ids >= 0).all() and env.status() == 0
        assert moves == [[int(x) for x in np.repeat(np.arange(3, 18), rows[a, :15].astype(int))] for a in ids]
