"""GPU (-m gpu): ddz_puct_open / _step / _close / ddz_puct_priors against search spec v5 (guided PUCT) restated on the CPU
oracle (tests/puct_reference.py).  visits, wins, the five totals and EVERY launch's leaf rows and need flags are compared
exactly.  Every reference is computed once per module and never written; the coverage conditions are read from the
references' traces and asserted (tests/test_puct_cpu.py asserts the same without a device)."""
import importlib
import os

import numpy as np
import pytest
import torch

import constructed_states as cs
import jk_cases as jc
import playout_reference as pr
import puct_cases as pc
import puct_reference as pp

pytestmark = pytest.mark.gpu
OUT_OF_DOMAIN = 64                                # status bit 6
FILL = 0x3F
COMBOS = [(h, s) for h in (False, True) for s in pc.SALTS]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


@pytest.fixture(scope="module")
def engine():
    return importlib.import_module("doudizhu-rl_amd.engine")


@pytest.fixture(scope="module")
def roots(oracle):
    table = cs.Table(*oracle.action_table())
    return {False: pc.build(oracle, table), True: pc.build(oracle, table, hidden=True)}


def _dev():
    return torch.device("cuda:0")


def _roles(hidden):
    return pc.ROLES_HIDDEN if hidden else 0b111


_refs = {}


def ref(oracle, roots, hidden, salt, pool=None):
    """(visits, wins, totals, launches, items) of the hashed evaluator, computed once"""
    k = (hidden, salt, pool)
    if k not in _refs:
        _refs[k] = pp.puct(oracle, roots[hidden], pc.BUDGET, pc.hash_eval, trees=pc.TREES, c=pc.C, seed=pc.SEED, gid_base=pc.GID_BASE,
                           salt=salt, hidden=hidden, roles=_roles(hidden), pool=pool, trace=True)
    return _refs[k]


def _env(pkg, states, seed=pc.SEED, gid_base=pc.GID_BASE, **kw):
    env = pkg.BatchedEnv(len(states), seed=seed, device=_dev(), table_id_base=gid_base, **kw)
    env.state_import(torch.from_numpy(np.ascontiguousarray(states).reshape(-1)))
    return env


class HostLeaf:
    """an evaluator computed on the host from the rows a launch left: keeps every launch's (leaf_rows, need)"""

    def __init__(self, fn):
        self.fn, self.launches = fn, []

    def __call__(self, search):
        rows, need = search.leaves.cpu().numpy().copy(), search.need.cpu().numpy().copy()
        i = len(self.launches)
        self.launches.append((rows, need))
        values, priors = self.fn(rows, need, i)
        search.values.copy_(torch.from_numpy(np.asarray(values).astype(np.int32)))
        search.priors.copy_(torch.from_numpy(np.ascontiguousarray(priors, dtype=np.uint8)))


def _run(env, leaf, budget=pc.BUDGET, **kw):
    totals = torch.zeros(5, dtype=torch.int64, device=_dev())
    visits, wins = env.guided_puct(budget, **kw).run(leaf, totals=totals)
    return visits.cpu().numpy(), wins.cpu().numpy(), totals.cpu().numpy()


def _same(got, want):
    for name, g, w in zip(("visits", "wins", "totals"), got, want[:3]):
        assert np.array_equal(g, w), (name, np.argwhere(np.asarray(g) != np.asarray(w))[:8].tolist(), np.asarray(g).sum(), np.asarray(w).sum())


def _exact(pkg, st, want, hidden, salt, pool=None, **kw):
    """one run on a pre-filled workspace against `want`: every launch, then the outputs -> (env, per-tree bytes)"""
    env = _env(pkg, st, **kw)
    per = env.lib.ddz_puct_work_bytes(1, pc.BUDGET, 1, pp.default_pool(pc.BUDGET) if pool is None else pool)
    env._puct_work = torch.full((per * len(st) * pc.TREES,), FILL, dtype=torch.uint8, device=_dev())
    leaf = HostLeaf(pc.hash_eval)
    got = _run(env, leaf, trees=pc.TREES, c=pc.C, salt=salt, hidden=hidden, roles=_roles(hidden), pool=pool)
    assert len(leaf.launches) == pc.BUDGET
    for i, ((rows, need), (wrows, wneed)) in enumerate(zip(leaf.launches, want[3])):
        assert np.array_equal(need, wneed), (i, need.tolist(), wneed.tolist())
        assert np.array_equal(rows, wrows), (i, np.argwhere(rows != wrows)[:8].tolist())
    _same(got, want)
    return env, per


@pytest.mark.parametrize("hidden,salt", COMBOS)
def test_exact_against_the_restatement(pkg, oracle, roots, hidden, salt):
    """the hashed evaluator (values in [-50, 1100], weights in four manners): every launch's rows and flags, then the outputs.
    The workspace is pre-filled: the trees of idle tables, of the table `roles` leaves out and of the one outside the domain
    keep every byte"""
    st = roots[hidden]
    env, per = _exact(pkg, st, ref(oracle, roots, hidden, salt), hidden, salt)
    assert env.status() == (OUT_OF_DOMAIN if hidden else 0)
    work = env._puct_work.view(len(st), pc.TREES * per).cpu().numpy()
    untouched = [pc.NOT_DEALT, pc.DONE] + ([pc.MASKED, pc.OUTSIDE] if hidden else [])
    assert (work[untouched] == FILL).all() and (work[[0, 1, pc.MID]] != FILL).any(1).all()


@pytest.mark.parametrize("hidden", (False, True))
def test_a_small_pool_falls_back_to_uniform(pkg, oracle, roots, hidden):
    """pool = 16: one short run fits, every later node is uniform and counted; still exact"""
    salt = pc.SALTS[1]
    want = ref(oracle, roots, hidden, salt, pc.SMALL_POOL)
    assert want[2][4] > 0
    env, per = _exact(pkg, roots[hidden], want, hidden, salt, pool=pc.SMALL_POOL)
    assert per == env.lib.ddz_puct_work_bytes(1, pc.BUDGET, 1, pp.default_pool(pc.BUDGET)) - pp.default_pool(pc.BUDGET) + 16


def test_coverage(oracle, roots):
    """what the references above walked through (their traces; nothing runs on the device here)"""
    for hidden in (False, True):
        items = [it for salt in pc.SALTS for it in ref(oracle, roots, hidden, salt)[4]]
        cover = pc.coverage(items, pc.BUDGET)
        assert all(cover.values()), (hidden, [k for k, v in cover.items() if not v])
        small = ref(oracle, roots, hidden, pc.SALTS[1], pc.SMALL_POOL)
        assert any(r["fallback"] for it in small[4] for r in it.iters)
    n_root = pr.root_lists(oracle, roots[True])[0]
    assert 64 < n_root[pc.MID] < pc.BUDGET


def test_the_joker_kicker_build(pkg, oracle):
    """k_puct<false> of libddz_hip_jk.so on the roots that hold joker-kicker rows, exact; the trees expand such rows"""
    build = importlib.import_module("doudizhu-rl_amd.build")
    if not os.path.exists(build.LIB_JK):
        pytest.skip("the joker-kicker build is absent")
    st = jc.roots(oracle)[0]
    salt = pc.SALTS[0]
    with oracle.variant(jk=True):
        want = pp.puct(oracle, st, pc.BUDGET, pc.hash_eval, trees=pc.TREES, c=pc.C, seed=pc.SEED, gid_base=pc.GID_BASE, salt=salt,
                       trace=True)
    assert sum(r["expand"] is not None and r["expand_id"] >= jc.NA_PLAIN for it in want[4] for r in it.iters) > 0
    env, _ = _exact(pkg, st, want, False, salt, native_joker_kickers=True)
    assert env.native_joker_kickers and env.status() == 0


def _priors_want(q, counts, role, running, inv, inv_tau, net_roles, before):
    """ddz_puct_priors stated in float64"""
    out = before.copy()
    for i in range(len(counts)):
        if not running[i] or not (net_roles >> role[i]) & 1:
            continue
        x = q[i, :counts[i]].astype(np.float64)
        if np.isnan(x).any():
            out[i, :counts[i]] = 1
            continue
        w = np.rint(255.0 * np.exp((x - x.max()) * float(np.float32(inv[role[i]])) * float(np.float32(inv_tau))))
        out[i, :counts[i]] = np.clip(w, 0, 255).astype(np.uint8)
    return out


def test_puct_priors_on_constructed_slabs(engine):
    """rows of 1, 63, 64, 65 and `stride` entries, the maximum at either end; an all-equal row; a NaN row; a role outside
    net_roles; rows that are not running.  One unit of tolerance against float64 (expf is good to a few ulp, far below 1 / 255:
    only a flip at a rounding boundary can occur); the maximum is 255 exactly; untouched rows and the tails keep their fill"""
    stride, inv, inv_tau = 512, (1.0, 0.5, 0.25), 0.75
    rng = np.random.default_rng(7)
    cases = []                                     # (role, n, q row)
    for role in (0, 1, 2):
        for n in (1, 63, 64, 65, stride):
            x = rng.normal(0.0, 3.0, n).astype(np.float32)
            for at in (0, n - 1):
                y = x.copy()
                y[at] = np.float32(y.max() + 1.5)
                cases.append((role, n, y))
        cases.append((role, 70, np.full(70, np.float32(-2.25))))          # all equal: every weight 255
        y = rng.normal(0.0, 3.0, 130).astype(np.float32)
        y[129] = np.nan
        cases.append((role, 130, y))                                       # a NaN: all ones
        cases.append((role, 40, (np.arange(40, dtype=np.float32) * np.float32(-0.75))))   # down to exp(-29): zeros at the end
    n = len(cases)
    q = np.full((n, stride), 99.0, np.float32)      # beyond the list: never read
    counts = np.zeros(n, np.int32)
    rows = np.zeros((n, 11, 16), np.uint8)
    for i, (role, cnt, x) in enumerate(cases):
        q[i, :cnt] = x
        counts[i] = cnt
        rows[i, cs.F_META, cs.M_ROLE], rows[i, cs.F_META, pr.M_DEALT], rows[i, cs.F_META, pr.M_WINNER] = role, 1, 0xFF
    rows[1, cs.F_META, pr.M_DEALT] = 0             # not dealt: untouched
    rows[2, cs.F_META, cs.M_DONE] = 1              # done: untouched
    role = rows[:, cs.F_META, cs.M_ROLE].astype(np.int64)
    running = (rows[:, cs.F_META, pr.M_DEALT] != 0) & (rows[:, cs.F_META, cs.M_DONE] == 0)
    dq, dc, dr = (torch.from_numpy(x).to(_dev()) for x in (q, counts, rows))
    seen = set()
    for net_roles in (0b111, 0b010, 0b101):
        before = np.full((n, stride), 0xA5, np.uint8)
        out = torch.from_numpy(before).to(_dev())
        got = engine.puct_priors(dr, dc, dq, inv, inv_tau=inv_tau, net_roles=net_roles, out=out).cpu().numpy()
        want = _priors_want(q, counts, role, running, inv, inv_tau, net_roles, before)
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        print("ddz_puct_priors: net_roles", net_roles, "largest difference", diff.max(), "entries off by one", int((diff == 1).sum()))
        assert diff.max() <= 1, np.argwhere(diff > 1)[:8].tolist()
        for i in range(n):
            taken = running[i] and (net_roles >> role[i]) & 1
            assert (got[i, counts[i]:] == 0xA5).all()
            if not taken:
                assert (got[i] == 0xA5).all()
            elif np.isnan(q[i, :counts[i]]).any():
                assert (got[i, :counts[i]] == 1).all()
            else:
                top = q[i, :counts[i]] == q[i, :counts[i]].max()
                assert (got[i, :counts[i]][top] == 255).all()
                seen |= set(got[i, :counts[i]].tolist())
    assert {0, 1, 255} <= seen and len(seen) > 100


def test_playout_leaf_end_to_end(pkg, oracle, roots):
    """guided_puct(24, trees=2).run(PlayoutLeaf(4)) against the restatement fed playout_reference's counts with the same two
    formulas, integer-exact: the weights come from the scratch environment's slab and are consumed in ply_list order, so a
    list order that differed between the two would show"""
    K, budget, salt = 4, 24, 9
    st = roots[False]
    want = pp.puct(oracle, st, budget, pp.playout_leaf(oracle, K, seed=pc.SEED, salt=salt), trees=pc.TREES, c=pc.C, seed=pc.SEED,
                   gid_base=pc.GID_BASE, salt=1, trace=True)
    env = _env(pkg, st)
    leaf = pkg.PlayoutLeaf(K, salt=salt)
    got = _run(env, leaf, budget=budget, trees=pc.TREES, c=pc.C, salt=1)
    _same(got, want)
    sums = {r["S"] for it in want[4] for r in it.iters if r["pending"]}
    assert want[0].sum() == (budget - 1) * pc.TREES * 4 and len(sums) > 10       # the weights differ from node to node
    assert any(len(set(it.pool[:it.nodes[0].n].tolist())) > 1 for it in want[4])  # and within a list
    assert leaf.env.T == len(st) * pc.TREES and env.status() == 0 and leaf.env.status() == 0


def test_guided_puct_choose_takes_the_most_visits(pkg, oracle, roots):
    st = roots[False]
    want = ref(oracle, roots, False, pc.SALTS[0])
    n, off, ids = pr.root_lists(oracle, st)
    env = _env(pkg, st)
    got = env.guided_puct_choose(HostLeaf(pc.hash_eval), pc.BUDGET, trees=pc.TREES, c=pc.C, salt=pc.SALTS[0]).cpu().numpy()
    for t in (0, 1, pc.MID, pc.MASKED):
        assert got[t] == ids[off[t] + int(np.argmax(want[0][t, :n[t]]))], t
    assert env.status() == 0


def test_misuse_is_refused_without_a_launch(pkg, roots):
    """mode "reference", a misaligned priors and a bad pool: ValueError or the argument code, nothing written; one open search
    per environment, shared with guided()"""
    st = roots[False]
    env = _env(pkg, st)
    env.legal_slab()
    L, T, stride = env.lib, env.T, env.slab_stride
    n = T * pc.TREES
    pool = pp.default_pool(64)
    nbytes = L.ddz_puct_work_bytes(T, 64, pc.TREES, pool)
    work = torch.full((nbytes,), FILL, dtype=torch.uint8, device=_dev())
    rows = torch.full((n * 176,), FILL, dtype=torch.uint8, device=_dev())
    need = torch.full((n,), -5, dtype=torch.int32, device=_dev())
    vals = torch.zeros(n, dtype=torch.int32, device=_dev())
    pri = torch.zeros(n * stride + 16, dtype=torch.uint8, device=_dev())
    v = torch.full((T * stride,), -5, dtype=torch.int32, device=_dev())
    head = (64, pc.TREES)
    tail = (1.25, 0, 0, 7)
    assert L.ddz_puct_open(env._h, *head, 0, *tail, stride, pool, work.data_ptr(), nbytes, None) == -1                   # the mode
    assert L.ddz_puct_step(env._h, *head, 0, *tail, stride, pool, vals.data_ptr(), pri.data_ptr(), rows.data_ptr(), need.data_ptr(),
                           work.data_ptr(), nbytes, None) == -1
    assert L.ddz_puct_close(env._h, *head, 0, *tail, vals.data_ptr(), pri.data_ptr(), stride, pool, v.data_ptr(), v.data_ptr(), None,
                            work.data_ptr(), nbytes, None) == -1
    assert L.ddz_puct_step(env._h, *head, 1, *tail, stride, pool, vals.data_ptr(), pri.data_ptr() + 8, rows.data_ptr(),
                           need.data_ptr(), work.data_ptr(), nbytes, None) == -1                                          # 16-byte priors
    assert L.ddz_puct_close(env._h, *head, 1, *tail, vals.data_ptr(), pri.data_ptr() + 4, stride, pool, v.data_ptr(), v.data_ptr(),
                            None, work.data_ptr(), nbytes, None) == -1
    for bad in (0, 8, 24, -16, (1 << 24) + 16):                                                                          # the pool
        assert L.ddz_puct_open(env._h, *head, 1, *tail, stride, bad, work.data_ptr(), nbytes, None) == -1
        assert L.ddz_puct_work_bytes(T, 64, pc.TREES, bad) == -1
    assert L.ddz_puct_open(env._h, *head, 1, *tail, stride, pool, work.data_ptr(), nbytes - 1, None) == -4               # DDZ_ECAP
    assert L.ddz_puct_open(env._h, *head, 1, *tail, stride, pool + 16, work.data_ptr(), nbytes, None) == -4
    assert L.ddz_puct_open(env._h, 4096, 512, 1, *tail, stride, pool, work.data_ptr(), 1 << 60, None) == -1              # 2^31
    torch.cuda.synchronize()
    assert (work == FILL).all() and (rows == FILL).all() and (need == -5).all() and (v == -5).all() and env.status() == 0
    for kw in (dict(mode="reference"), dict(pool=24), dict(pool=0), dict(pool=(1 << 24) + 16)):
        with pytest.raises(ValueError):
            env.guided_puct(8, trees=pc.TREES, **kw)
    s = env.guided_puct(8, trees=pc.TREES)
    assert s.priors.shape == (n, stride) and s.priors.dtype == torch.uint8 and s.pool == pp.default_pool(8)
    with pytest.raises(RuntimeError):
        env.guided_puct(8, trees=pc.TREES)
    with pytest.raises(RuntimeError):
        env.guided(8, trees=pc.TREES)
    s.step()
    for name, bad in (("priors", torch.zeros((n, stride), dtype=torch.int8, device=_dev())),
                      ("priors", torch.zeros((n, stride - 1), dtype=torch.uint8, device=_dev())),
                      ("priors", torch.zeros((n, stride), dtype=torch.uint8))):
        keep = getattr(s, name)
        setattr(s, name, bad)
        with pytest.raises(ValueError):
            s.step()
        with pytest.raises(ValueError):
            s.close()
        setattr(s, name, keep)
    with pytest.raises(ValueError):
        s.close(torch.zeros(4, dtype=torch.int64, device=_dev()))        # five totals
    assert s.steps == 1 and not s.closed
    s.close(torch.zeros(5, dtype=torch.int64, device=_dev()))
    g = env.guided(8, trees=pc.TREES)                                     # closed: the environment is free again
    with pytest.raises(RuntimeError):
        env.guided_puct(8, trees=pc.TREES)
    g.close()
    assert env.status() == 0


def test_a_header_open_did_not_write_runs_nothing(pkg, roots):
    """a step and a close on a workspace no open wrote, or on one whose pool mark is out of range, touch nothing of it, emit
    all-zero rows and flags and add nothing to the root sums or the totals"""
    st = roots[False]
    env = _env(pkg, st)
    env.legal_slab()
    L, T, stride = env.lib, env.T, env.slab_stride
    budget, n, pool = 16, env.T * pc.TREES, 64
    nbytes = L.ddz_puct_work_bytes(T, budget, pc.TREES, pool)
    per = nbytes // n
    common = (budget, pc.TREES, 1, 1.25, 0, 0, 7)

    def step_and_close(work):
        rows = torch.full((n * 176,), FILL, dtype=torch.uint8, device=_dev())
        need = torch.full((n,), -5, dtype=torch.int32, device=_dev())
        vals = torch.full((n,), 700, dtype=torch.int32, device=_dev())
        pri = torch.full((n * stride,), 9, dtype=torch.uint8, device=_dev())
        v, w = (torch.zeros(T * stride, dtype=torch.int32, device=_dev()) for _ in range(2))
        totals = torch.zeros(5, dtype=torch.int64, device=_dev())
        assert L.ddz_puct_step(env._h, *common, stride, pool, vals.data_ptr(), pri.data_ptr(), rows.data_ptr(), need.data_ptr(),
                               work.data_ptr(), nbytes, None) == 0
        assert L.ddz_puct_close(env._h, *common, vals.data_ptr(), pri.data_ptr(), stride, pool, v.data_ptr(), w.data_ptr(),
                                totals.data_ptr(), work.data_ptr(), nbytes, None) == 0
        torch.cuda.synchronize()
        return not rows.any() and not need.any() and not v.any() and not w.any() and not totals.any()

    for fill in (FILL, 0):
        work = torch.full((nbytes,), fill, dtype=torch.uint8, device=_dev())
        assert step_and_close(work) and (work == fill).all()
    for word, value in ((12, pool + 4), (12, 2), (1, budget + 1), (3, 1)):      # the pool mark beyond the pool / unaligned; spec v3's
        work = torch.full((nbytes,), FILL, dtype=torch.uint8, device=_dev())
        assert L.ddz_puct_open(env._h, *common, stride, pool, work.data_ptr(), nbytes, None) == 0
        hdr = work.view(n, per)[:, :64].contiguous().view(torch.int32)
        assert hdr[[0, pc.TREES, pc.TREES * pc.MID], 0].tolist() == [1, 1, 1]
        hdr[:, word] = value
        work.view(n, per)[:, :64] = hdr.view(torch.uint8)
        kept = work.clone()
        assert step_and_close(work) and torch.equal(work, kept), (word, value)
    assert env.status() == 0


Q_REWARD = {"up": 0.5, "lord": 1.0, "down": 0.5}   # (small rewards: an untrained network's values spread over many units)


def test_qleaf_fills_values_and_priors(pkg, engine, roots):
    """dqn_glue.QLeaf(tau=0.5) on a search with priors: every waiting item's weights against ddz_puct_priors' formula in
    float64 on the q slab QLeaf itself computes (one unit of tolerance), the best move 255; tails and idle items keep a fill"""
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    variant, st = 3, roots[False]
    nets = {}
    for role, seed in (("up", 11), ("lord", 12), ("down", 13)):
        torch.manual_seed(seed)
        nets[role] = glue.QNet(engine.FACE_PLANES[variant]).to(_dev()).eval()
    inv = [1.0 / Q_REWARD[r] for r in glue.ROLE_ORDER]
    qleaf = glue.QLeaf(nets, variant, reward_dict=Q_REWARD, tau=0.5)
    with pytest.raises(ValueError):
        glue.QLeaf(nets, variant, tau=0.0)
    env = _env(pkg, st)
    search = env.guided_puct(6, trees=pc.TREES)
    waited, spread = 0, set()
    for i in range(6):
        search.step()
        search.priors.fill_(0xA5)
        values = qleaf(search).cpu().numpy()
        q, scratch = qleaf.q_values(search)
        q, counts = q.cpu().numpy().reshape(search.n_items, -1), scratch.counts.cpu().numpy()
        rows, need, got = search.leaves.cpu().numpy(), search.need.cpu().numpy(), search.priors.cpu().numpy()
        assert (got[need == 0] == 0xA5).all()
        for k in np.flatnonzero(need):
            n, role = int(counts[k]), int(rows[k, cs.F_META, cs.M_ROLE])
            x = q[k, :n].astype(np.float64)
            want = np.clip(np.rint(255.0 * np.exp((x - x.max()) * float(np.float32(inv[role])) * 2.0)), 0, 255)
            assert n > 0 and np.abs(got[k, :n].astype(np.int64) - want).max() <= 1 and got[k, int(x.argmax())] == 255
            assert (got[k, n:] == 0xA5).all() and 0 <= values[k] <= 1024
            waited += 1
            spread |= set(got[k, :n].tolist())
    search.close()
    assert waited > 30 and len(spread) > 20 and env.status() == 0 and qleaf.loop.env.status() == 0


def test_teacher_and_serving(pkg, oracle, roots):
    """Teacher("guided_puct") hands guided()'s kind of root statistics (visits, wins in 1024ths) and chooses by visits;
    serving.guided_puct_act answers with guided_puct_choose's move in the hidden form"""
    serving = importlib.import_module("doudizhu-rl_amd.serving")
    st = roots[False]
    env = _env(pkg, st)
    kw = dict(budget=16, trees=pc.TREES, salt=5)
    teacher = pkg.Teacher("guided_puct", evaluator=pkg.PlayoutLeaf(2, salt=1), **kw)
    stats = teacher.evaluate(env)
    den, num = stats.den.view(env.T, -1).cpu().numpy(), stats.num.view(env.T, -1).cpu().numpy()
    assert stats.scale == 1024 and stats.den_const is None
    assert den.sum(1).tolist() == [15 * pc.TREES if t in (0, 1, pc.MID, pc.MASKED) else 0 for t in range(env.T)]
    assert (num <= den * 1024).all() and (num >= 0).all()
    ids = teacher.choose(env, stats).cpu().numpy()
    n, off, lst = pr.root_lists(oracle, st)
    for t in (0, 1, pc.MID, pc.MASKED):
        assert ids[t] == lst[off[t] + int(np.argmax(den[t, :n[t]]))]
    again = env.guided_puct_choose(pkg.PlayoutLeaf(2, salt=1), 16, trees=pc.TREES, salt=5).cpu().numpy()
    assert np.array_equal(again, ids)
    with pytest.raises(ValueError):
        pkg.Teacher("guided_puct", budget=16)                      # no evaluator
    # serving: plain payloads, the hidden form
    sub = st[[0, 1, pc.MID, pc.MASKED]]
    payloads = serving.state_to_full_payloads(sub)
    rows = pkg.action_table(_dev()).cpu().numpy()
    moves = serving.guided_puct_act(payloads, pkg.PlayoutLeaf(2, salt=1), 16, device=_dev(), salt=5, trees=2)
    env2 = _env(pkg, serving.payloads_to_playout_state(payloads), 0, 0)
    ids2 = env2.guided_puct_choose(pkg.PlayoutLeaf(2, salt=1), 16, trees=2, salt=5, hidden=True).cpu().numpy()
    assert (ids2 >= 0).all() and env2.status() == 0
    assert moves == [[int(x) for x in np.repeat(np.arange(3, 18), rows[a, :15].astype(int))] for a in ids2]
