"""GPU (-m gpu): the entry into a table that the seven evaluator kernels k_playout, k_search, k_cfr, k_solve, k_ismcts, k_guided
and k_gismcts share (csrc/ddz_ply.h: table_enter, root_hands), held to the seven references on that entry alone.  One batch of six tables, one per way a table can go through it:
  0 not dealt          1 done          2 running, its actor outside `roles`
  3 running, outside the hidden-hand domain (five cards: below every card limit)
  4 outside the domain AND above the solvers' card limit (nine cards: the limit is tested first, no status bit from them)
  5 running and inside
in that order and in reverse, every output the verb does not zero itself filled with a sentinel (for the two guided verbs:
the workspace before the open, the leaf rows and need flags before every step), everything compared exactly (integers;
sigma / value as bit patterns; every launch's leaf rows and flags) with the status word.  Table 4 raises bit 6 in the three
tree searches that know no card limit (ismcts, guided in its hidden form, gismcts) as it does in search.  Then the batch without table 3, where bit 6 must stay clear
for the two solvers, and the inside table alone and repeated over one block and a wave: the `t >= T` leave behind the
block's barrier.  The settings are small on purpose: nothing here tests the loops behind the entry."""
import importlib

import numpy as np
import pytest
import torch

import cfr_reference as cr
import gismcts_reference as gir
import guided_reference as gr
import ismcts_reference as ir
import playout_hidden_cases as hc
import playout_hidden_reference as phr
import search_reference as sr
import solve_cases as sc
import solve_reference as sv

pytestmark = pytest.mark.gpu
SEED, GID_BASE, SALT = 13, 2 ** 32 + 5, 3
ROLES = 0b010                                     # the lord's tables take part
SENTINEL = 0x3F3F3F3F
DOMAIN = 64                                       # status bit 6
VERBS = ("playout", "search", "cfr", "solve", "ismcts", "guided", "gismcts")
WAVES = {"playout": 12, "search": 12, "cfr": 4, "solve": 8, "ismcts": 12, "guided": 12, "gismcts": 12}   # wavefronts per block
TREES = dict(budget=4, trees=2)                   # the three tree searches added behind the four
FILL = 0x3F
SOLVE = dict(budget=40, max_cards=6, worlds=2, hidden=True, roles=ROLES, salt=SALT, chunks=2, tt_entries=16)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def six(oracle):
    states, names, _ = sc.batch(oracle)
    assert names[-4:] == ["idle: done", "idle: not dealt", "outside: 13 cards", "outside the hidden form: pool and hands differ"]
    inside, other_seat, done, fresh, short = states[2], states[3], states[-4], states[-3], states[-1]
    big = hc.out_of_domain()[1][2]                # "sizes one short" on a table of nine cards
    st = np.stack([fresh, done, other_seat, short, big, inside])
    role, cards = st[:, sc.F_META, sc.M_ROLE], st[:, :3, 15].astype(int).sum(1)
    assert role[2] != 1 and (role[3:] == 1).all() and cards[3] <= 6 < cards[4] and cards[5] <= 6
    return st


# ---- the references: {name: array}, status ----
_refs = {}


def ref(oracle, verb, st):
    k = (verb, oracle.num_actions(), st.tobytes())
    if k not in _refs:
        bad = phr.worlds(oracle, st, 2, SEED, GID_BASE, SALT, ROLES)[2]
        if verb == "playout":
            wins, totals, bad = phr.playouts_hidden(oracle, st, 2, SEED, GID_BASE, SALT, ROLES)
            _refs[k] = {"wins": wins, "totals": totals}, DOMAIN * int(bad.any())
        elif verb == "search":
            visits, wins, totals = sr.search(oracle, st, 4, trees=2, seed=SEED, gid_base=GID_BASE, salt=SALT, hidden=True, roles=ROLES)
            _refs[k] = {"visits": visits, "wins": wins, "totals": totals}, DOMAIN * int(bad.any())
        elif verb == "cfr":
            n, ids, sigma, value, totals, status, _ = cr.cfr(oracle, st, 1, roles=ROLES)
            _refs[k] = {"n": n, "ids": ids, "sigma": sigma, "value": value, "totals": totals}, status
        elif verb == "solve":
            n, wins, unknown, totals, status = sv.spec(oracle, st, seed=SEED, gid_base=GID_BASE, **SOLVE)
            _refs[k] = {"n": n, "wins": wins, "unknown": unknown, "totals": totals}, status
        elif verb == "ismcts":
            visits, wins, totals = ir.ismcts(oracle, st, TREES["budget"], trees=TREES["trees"], seed=SEED, gid_base=GID_BASE, salt=SALT,
                                             roles=ROLES)
            _refs[k] = {"visits": visits, "wins": wins, "totals": totals}, DOMAIN * int(bad.any())
        else:
            kw = dict(trees=TREES["trees"], seed=SEED, gid_base=GID_BASE, salt=SALT, roles=ROLES)
            if verb == "guided":
                visits, wins, totals, launches = gr.guided(oracle, st, TREES["budget"], gr.hash_leaf, hidden=True, **kw)
            else:
                visits, wins, totals, launches = gir.gismcts(oracle, st, TREES["budget"], gr.hash_leaf, **kw)
            _refs[k] = {"visits": visits, "wins": wins, "totals": totals, "leaves": np.stack([r for r, _ in launches]),
                        "need": np.stack([n for _, n in launches])}, DOMAIN * int(bad.any())
    return _refs[k]


# ---- the device ----
def run(pkg, verb, st):
    env = pkg.BatchedEnv(len(st), seed=SEED, device=_dev(), table_id_base=GID_BASE)
    env.state_import(torch.from_numpy(np.ascontiguousarray(st).reshape(-1)))
    T, S = env.T, env.slab_stride
    totals = torch.zeros(4, dtype=torch.int64, device=_dev())
    full = lambda shape, dt=torch.int32, v=SENTINEL: torch.full(shape, v, dtype=dt, device=_dev())
    if verb == "playout":               # (wins, and the visits / wins of search, are zeroed by the verb)
        out = {"wins": env.playout(2, salt=SALT, chunks=2, totals=totals, hidden=True, roles=ROLES)}
    elif verb == "search":
        v, w = env.search(4, trees=2, salt=SALT, hidden=True, roles=ROLES, totals=totals)
        out = {"visits": v, "wins": w}
    elif verb == "cfr":
        o = (full((T,)), full((T, 16)), full((T, 16), torch.float64, -7.0), full((T,), torch.float64, -7.0))
        out = dict(zip(("n", "ids", "sigma", "value"), env.cfr(1, roles=ROLES, totals=totals, out=o)))
    elif verb == "solve":               # (wins / unknown are zeroed by the verb, n is not)
        o = (full((T,)), full((T * S,)), full((T * S,)))
        out = dict(zip(("n", "wins", "unknown"), env.solve(out=o, totals=totals, **SOLVE)))
    elif verb == "ismcts":              # (visits / wins are zeroed by the verb; the trees' workspace is not)
        need = env.lib.ddz_ismcts_work_bytes(T, TREES["budget"], TREES["trees"])
        env._ismcts_work = full((need,), torch.uint8, FILL)
        v, w = env.ismcts(salt=SALT, roles=ROLES, totals=totals, **TREES)
        out = {"visits": v, "wins": w}
    else:                               # (visits / wins are zeroed by close; the workspace, the leaf rows and the flags are not)
        items = T * TREES["trees"]
        if verb == "guided":
            env._guided_work = full((env.lib.ddz_guided_work_bytes(T, TREES["budget"], TREES["trees"]),), torch.uint8, FILL)
            s = env.guided(salt=SALT, hidden=True, roles=ROLES, **TREES)
        else:
            env._gismcts_work = full((env.lib.ddz_gismcts_work_bytes(T, TREES["budget"], TREES["trees"]),), torch.uint8, FILL)
            s = env.guided_ismcts(salt=SALT, roles=ROLES, **TREES)
        leaves, flags = [], []
        for i in range(TREES["budget"]):
            s.leaves.fill_(FILL)
            s.need.fill_(SENTINEL)
            s.step()
            rows, need = s.leaves.cpu().numpy().copy(), s.need.cpu().numpy().copy()
            leaves.append(torch.from_numpy(rows))
            flags.append(torch.from_numpy(need))
            assert need.shape == (items,) and set(need.tolist()) <= {0, 1}           # (nothing else can index the evaluator)
            if need.any():
                s.values.copy_(torch.from_numpy(np.asarray(gr.hash_leaf(rows, need, i)).astype(np.int32)))
        v, w = s.close(totals)
        out = {"visits": v, "wins": w, "leaves": torch.stack(leaves), "need": torch.stack(flags)}
    torch.cuda.synchronize()
    out["totals"] = totals
    return {k: x.cpu().numpy() for k, x in out.items()}, env.status()


def check(pkg, oracle, verb, st):
    (want, status), (got, got_status) = ref(oracle, verb, st), run(pkg, verb, st)
    assert set(got) == set(want)
    for name, w in want.items():
        g, w = np.asarray(got[name]), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), (verb, name, np.argwhere(g != w)[:8].tolist())
    assert got_status == status, verb
    return want, status


@pytest.mark.parametrize("order", ["in order", "reversed"])
@pytest.mark.parametrize("verb", VERBS)
def test_six_tables(pkg, oracle, six, verb, order):
    st = six if order == "in order" else six[::-1].copy()
    want, status = check(pkg, oracle, verb, st)
    at = (lambda t: t) if order == "in order" else (lambda t: 5 - t)
    assert status == DOMAIN                      # the fourth table raises it in every kernel
    if verb in ("cfr", "solve"):                 # what the reference says of the six, before it is believed
        assert [int(want["n"][at(t)]) for t in range(5)] == [0, 0, 0, -1, -1] and want["n"][at(5)] > 0
    rows = want["visits" if "visits" in want else "wins" if verb != "cfr" else "sigma"]
    assert not rows[[at(t) for t in range(5)]].any() and rows[at(5)].any()


@pytest.mark.parametrize("verb", VERBS)
def test_the_card_limit_stands_before_the_domain(pkg, oracle, six, verb):
    """without the fourth table: the fifth is outside the domain and above the limit -- no status bit from the two solvers"""
    _, status = check(pkg, oracle, verb, np.delete(six, 3, axis=0))
    assert status == (0 if verb in ("cfr", "solve") else DOMAIN)


@pytest.mark.parametrize("tables", ["one table", "a block and a wave"])
@pytest.mark.parametrize("verb", VERBS)
def test_block_edges(pkg, oracle, six, verb, tables):
    T = 1 if tables == "one table" else WAVES[verb] + 1
    want, status = check(pkg, oracle, verb, np.repeat(six[5:6], T, axis=0))      # (worlds and trees are keyed by the table id)
    assert status == 0
    if verb in ("cfr", "solve"):
        assert (want["n"] > 0).all()
