"""GPU (-m gpu): k_playout ply by ply on the constructed roots of tests/playout_cases.py, in both builds, and
k_playout_choose on constructed buffers, against tests/playout_reference.py.  What the playouts from these roots walk through
is asserted on the reference's trace by tests/test_playout_cases_cpu.py.  Every comparison is exact integer equality; the
references are computed once per module and never written."""
import importlib

import numpy as np
import pytest
import torch

import constructed_states as cs
import playout_cases as pc
import playout_reference as pr

pytestmark = pytest.mark.gpu
CHUNKS = (1, 3, 4, 7, 12, 1000)
GARBAGE = 0x5A5A5A5A


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


@pytest.fixture(scope="module")
def plain(oracle):
    table = cs.Table(*oracle.action_table())
    sets = pc.build(oracle, table)
    return sets, {n: pc.reference(oracle, s) for n, s in sets.items()}


@pytest.fixture(scope="module")
def jk(oracle):
    with oracle.variant(jk=True):
        sets = pc.build(oracle, cs.Table(*oracle.action_table()), jk=True)
        return sets, {n: pc.reference(oracle, s) for n, s in sets.items()}


def _dev():
    return torch.device("cuda:0")


def _env(pkg, s, states=None, **kw):
    env = pkg.BatchedEnv(s.T, seed=s.seed, device=_dev(), table_id_base=s.gid_base, **kw)
    env.state_import(torch.from_numpy(np.ascontiguousarray(s.states if states is None else states).reshape(-1)))
    return env


def _run(env, K, **kw):
    totals = torch.zeros(4, dtype=torch.int64, device=_dev())
    wins = env.playout(K, totals=totals, **kw)
    return wins.cpu().numpy(), totals.cpu().numpy()


def _whole(pkg, s, ref, **kw):
    """the whole batch in one launch: wins [T, stride] and totals as the reference has them, the lists as long"""
    env = _env(pkg, s, **kw)
    wins, totals = _run(env, s.K)
    assert np.array_equal(wins, ref[0]) and np.array_equal(totals, ref[1]), s.name
    assert totals[2] == 0 and env.status() == 0
    return env


@pytest.mark.parametrize("name", ["roots", "ply", "deals"])
def test_constructed_roots(pkg, oracle, plain, name):
    s, (wins, totals, tr) = plain[0][name], plain[1][name]
    env = _whole(pkg, s, (wins, totals))
    n = pr.root_lists(oracle, s.states, s.seed, s.gid_base)[0]
    assert np.array_equal(env.legal_slab()[0].cpu().numpy(), n)
    # table by table: every other table never dealt (the table keeps its index and so its gid), one launch each with totals of
    # its own -- the moves applied by the playouts of THIS root
    got_w = torch.zeros((s.T, env.slab_stride), dtype=torch.int32, device=_dev())
    got_t = torch.zeros((s.T, 4), dtype=torch.int64, device=_dev())
    alone = torch.zeros((s.T, 176), dtype=torch.uint8)
    for t in range(s.T):
        alone.zero_()
        alone[t] = torch.from_numpy(s.states[t].reshape(-1))
        env.state_import(alone)
        w = env.playout(s.K, totals=got_t[t])
        got_w[t] = w[t]
        w[t] = 0
        got_t[t, 3] = w.ne(0).sum()                   # (nothing but this table's row is written)
    got_w, got_t = got_w.cpu().numpy(), got_t.cpu().numpy()
    assert env.status() == 0
    bad = [s.names[t] for t in range(s.T) if got_t[t, 1] != n[t] * s.K]
    assert not bad, "imported as not running, or another list: " + "; ".join(bad[:5])
    bad = [s.names[t] for t in range(s.T) if got_t[t, 0] != tr.moves_per_table[t] or not np.array_equal(got_w[t], wins[t])]
    assert not bad, "moves applied or wins differ: " + "; ".join(bad[:5])
    assert not got_t[:, 2:].any()


def test_long_list(pkg, oracle, plain):
    s = plain[0]["long"]
    env = _whole(pkg, s, plain[1]["long"][:2])
    n = env.legal_slab()[0].cpu().numpy()
    assert n[0] >= pc.LONG_MIN and np.array_equal(n, pr.root_lists(oracle, s.states)[0])


def test_outside_the_domain(pkg, oracle, plain):
    """a running table whose actor's hand is empty: the empty list -- nothing runs, wins stay zero, totals are unchanged"""
    s, ref = plain[0]["outside"], plain[1]["outside"]
    assert tuple(s.names) == pc.OUTSIDE
    env = _env(pkg, s)
    totals = torch.tensor([11, 22, 33, 44], dtype=torch.int64, device=_dev())
    wins = env.playout(s.K, totals=totals)
    assert not wins.any().item() and totals.tolist() == [11, 22, 33, 44] and env.status() == 0
    listed = pr.root_lists(oracle, s.states, s.seed, s.gid_base)[0] > 0     # where the oracle lists a move, the two differ by
    keep = ~listed                                                          # design: those of the two cases are left out
    assert np.array_equal(wins.cpu().numpy()[keep], ref[0][keep])


@pytest.mark.parametrize("T", [1, 5, 13])
def test_mapping(pkg, oracle, plain, T):
    s = pc.mapping_batch(plain[0], T)
    want = pr.playouts(oracle, s.states, s.K, seed=s.seed, gid_base=s.gid_base)
    assert want[1][2] == 0
    env = _env(pkg, s)
    n = env.legal_slab()[0].cpu().numpy().astype(np.int64)
    beyond = np.arange(env.slab_stride)[None, :] >= n[:, None]
    for chunks in CHUNKS:
        buf = torch.full((T * env.slab_stride,), GARBAGE, dtype=torch.int32, device=_dev())
        got = _run(env, s.K, chunks=chunks, wins=buf)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), chunks
        assert not buf.view(T, -1).cpu().numpy()[beyond].any(), chunks
    assert env.status() == 0


@pytest.mark.parametrize("T", [1, 6, 9])
def test_choose_on_constructed_buffers(pkg, T):
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    env = pkg.BatchedEnv(T, seed=1, device=_dev())
    stride = env.slab_stride
    assert stride == pr.STRIDE
    out = torch.empty(T, dtype=torch.int32, device=_dev())
    for name, counts, ids, wins, want, _ in pc.choose_problems(T, stride):
        d = [torch.from_numpy(x).to(_dev()) for x in (counts, ids, wins)]
        out.fill_(-7)
        rc = env.lib.ddz_playout_choose(env._h, engine._p(d[0]), engine._p(d[1]), stride, engine._p(d[2]), engine._p(out),
                                        engine._stream(_dev()))
        assert rc == 0
        assert np.array_equal(out.cpu().numpy(), want), (name, counts.tolist())
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(d, (counts, ids, wins))), name
    assert env.status() == 0


@pytest.mark.parametrize("name", ["roots", "jk leads", "jk deals"])
def test_joker_kicker_build(pkg, jk, name):
    s, ref = jk[0][name], jk[1][name]
    env = _whole(pkg, s, ref[:2], native_joker_kickers=True)
    assert env.native_joker_kickers
