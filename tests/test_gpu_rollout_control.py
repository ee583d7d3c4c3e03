"""GPU (-m gpu): the three wave-uniform tests of k_rollout's iteration body -- the refill of the 64 draws (`dnext >= 64`),
the idle iteration (`n <= 0`) and the win (`won`, with the deal behind it) -- where they fall inside a launch and on its first
and last iteration.  Everything is bytes and integers against OracleEnv: every comparison is exact.

  refill   From reset(), the same 70 iterations as one launch of 70, as launches of 63 + 1 + 6 and as 70 launches of 1: a launch
           starts with a refill, and a table whose episode is still running 64 plies later refills in the middle of the
           launch of 70 (ply 64) -- in the other two splits that ply falls on the first iteration of a launch.  6,144 tables
           (the smallest count that selects the dense 12-wave variant) and 256 tables (16-wave blocks).  With the seeds below
           2,239 of 6,144 tables (36.4 %) and 92 of 256 (35.9 %) are still in their first episode after 65 iterations; the
           oracle run asserts that there are some.  Forms: plain, with records (the last 6 iterations' records: they hold the
           draw of ply 64), and the staged-CSR rollout (its batches are the launches), without and with records.
  win      The oracle's state before the iteration of that run in which the most tables win (and some win in the one after):
           launches of 1 and of 2 iterations from it, with and without records -- win and deal on the only, the first and the
           last iteration of a launch.
  idle     Among the 6,144 tables a few states whose actor's hand is empty (deliberately foreign: no deal leads there; built
           from constructed_states.lead_exact with the actor's cards moved to its history).  The oracle defines the case --
           an empty list, nothing applied, the record flagged 2 -- so the comparison is against it: count 0, the state rows
           unchanged, plies = iterations - idle, status() == 0, and the neighbours play on as if nothing were there.

The oracle runs once per table count and is never written."""
import numpy as np
import pytest
import torch

import constructed_states as cs

pytestmark = pytest.mark.gpu
ITERS = 70
SPLITS = {"one": (70,), "edges": (63, 1, 6), "single": (1,) * 70}
RECORDED = 6                 # the oracle steps the last RECORDED iterations one by one (lists, records); the rest multi-threaded
THREADS = 16
WORLDS = {6144: (51, 2 ** 35 + 11), 256: (52, 977)}   # tables: (seed, table_id_base)


@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


def _np(x):
    return x.cpu().numpy()


def _steps(oracle, ref, n):
    """n iterations of the oracle one by one -> per iteration (list sizes, rows, records, wins), and the legal rows"""
    out, rows_sum = [], 0
    for _ in range(n):
        off, rows, _ = ref.legal()
        sizes, rows = np.diff(off).copy(), rows.copy()
        rows_sum += int(off[-1])
        done, _, _, traj = ref.step(oracle.STEP_RANDOM, auto_reset=True, want_traj=True)
        out.append({"sizes": sizes, "rows": rows, "traj": traj, "wins": int(done.sum()), "state": ref.state.copy()})
    return out, rows_sum


class Run:
    """the oracle's 70 iterations from reset() of one table count"""

    def __init__(self, oracle, T):
        self.T = T
        self.seed, self.base = WORLDS[T]
        ref = oracle.OracleEnv(T, seed=self.seed, gid_base=self.base)
        ref.reset()
        self.start = ref.state.copy()
        _, rows_sum, episodes = oracle.rollout_random_mt(ref, ITERS - RECORDED, THREADS)
        ply = cs.meta_ply(ref.state.reshape(T, cs.NFIELDS, cs.ROW))
        self.long = int((ply == ITERS - RECORDED).sum())      # tables still in their first episode after 64 iterations
        self.tail, rs = _steps(oracle, ref, RECORDED)
        self.longer = int((cs.meta_ply(self.tail[0]["state"].reshape(T, cs.NFIELDS, cs.ROW)) == ITERS - RECORDED + 1).sum())
        self.rows_sum = rows_sum + rs
        self.episodes = episodes + sum(s["wins"] for s in self.tail)
        self.state = ref.state.copy()


_runs = {}


def _run(oracle, T):
    if T not in _runs:
        _runs[T] = Run(oracle, T)
    return _runs[T]


def _lists(env, form):
    """(list sizes, the rows of all lists in table order) of the last iteration"""
    if "csr" in form:
        off = _np(env.offsets).astype(np.int64)
        return np.diff(off).astype(np.int32), _np(env.rows[:int(off[-1])])
    mask = torch.arange(env.slab_stride, device=_dev())[None, :] < env.counts[:, None]
    return _np(env.counts), _np(env.slab_rows()[mask])


@pytest.mark.parametrize("T,form", [(6144, "plain"), (256, "plain"), (6144, "records"), (6144, "csr"), (6144, "csr records")])
def test_refill_inside_and_at_the_edge_of_a_launch(pkg, oracle, T, form):
    r = _run(oracle, T)
    # the precondition: episodes that run past ply 64, so the launch of 70 refills its draws in the middle of an episode
    assert r.long > 0 and r.longer > 0, (r.long, r.longer)
    print(f"T {T}: {r.long} tables in their first episode after 64 iterations, {r.longer} after 65")
    last = r.tail[-1]
    got = {}
    for name, split in SPLITS.items():
        env = pkg.BatchedEnv(T, seed=r.seed, table_id_base=r.base, want_ids=False)
        env.reset()
        assert np.array_equal(_np(env.state), r.start)
        recs = []
        for n in split:
            traj = torch.zeros((n, T, 32), dtype=torch.uint8, device=_dev()) if "records" in form else None
            if "csr" in form:
                env.rollout_random_csr(n, traj=traj)
            else:
                env.rollout_random(n, traj=traj)
            if traj is not None:
                recs.append(traj)
        sizes, rows = _lists(env, form)
        got[name] = {"sizes": sizes, "rows": rows, "state": _np(env.state), "stats": env.stats()}
        if "records" in form:
            got[name]["traj"] = _np(torch.cat(recs))[ITERS - RECORDED:]
        assert env.status() == 0, name
    want = {"sizes": last["sizes"], "rows": last["rows"], "state": r.state}
    if "records" in form:
        want["traj"] = np.stack([s["traj"] for s in r.tail])
    for name, g in got.items():
        assert cs.differences(g, want) == [], (name, T, form)
        s = g["stats"]
        assert (s["plies"], s["legal_rows"], s["episodes"]) == (T * ITERS, r.rows_sum, r.episodes), (name, s)
        assert s["lord_wins"] + s["up_wins"] + s["down_wins"] == s["episodes"]
        assert s == got["one"]["stats"] and cs.differences(g, {k: v for k, v in got["one"].items() if k != "stats"}) == [], name


class Wins:
    """the state of the 6,144-table run before the iteration in which the most tables win, and the oracle's two iterations
    from it"""

    def __init__(self, oracle):
        T = 6144
        seed, base = WORLDS[T]
        ref = oracle.OracleEnv(T, seed=seed, gid_base=base)
        ref.reset()
        wins = []
        for it in range(40):       # finished episodes per iteration (multi-threaded, one iteration at a time)
            wins.append(oracle.rollout_random_mt(ref, 1, THREADS)[2])
        at = int(np.argmax(np.minimum(wins[:-1], wins[1:])))
        ref = oracle.OracleEnv(T, seed=seed, gid_base=base)
        ref.reset()
        if at:
            oracle.rollout_random_mt(ref, at, THREADS)
        self.T, self.seed, self.base, self.at = T, seed, base, at
        self.before = ref.state.copy()
        self.steps, _ = _steps(oracle, ref, 2)
        assert [s["wins"] for s in self.steps] == wins[at:at + 2]


_wins = []


@pytest.mark.parametrize("want_traj", [False, True])
@pytest.mark.parametrize("iters", [1, 2])
def test_win_and_deal_on_the_first_and_the_last_iteration(pkg, oracle, iters, want_traj):
    if not _wins:
        _wins.append(Wins(oracle))
    w = _wins[0]
    # the precondition: tables one ply from a win, and tables two plies from one
    assert w.steps[0]["wins"] >= 1 and w.steps[1]["wins"] >= 1, [s["wins"] for s in w.steps]
    print(f"iteration {w.at}: {w.steps[0]['wins']} tables win, {w.steps[1]['wins']} in the next")
    env = pkg.BatchedEnv(w.T, seed=w.seed, table_id_base=w.base, want_ids=False)
    env.state_import(torch.from_numpy(w.before))
    traj = torch.zeros((iters, w.T, 32), dtype=torch.uint8, device=_dev()) if want_traj else None
    env.rollout_random(iters, traj=traj)
    steps = w.steps[:iters]
    sizes, rows = _lists(env, "plain")
    got = {"sizes": sizes, "rows": rows, "state": _np(env.state)}
    want = {"sizes": steps[-1]["sizes"], "rows": steps[-1]["rows"], "state": steps[-1]["state"]}
    if want_traj:
        got["traj"], want["traj"] = _np(traj), np.stack([s["traj"] for s in steps])
    assert cs.differences(got, want) == []
    st = dict(cs.run_stats([s["traj"] for s in steps]), legal_rows=sum(int(s["sizes"].sum()) for s in steps))
    assert st["episodes"] == sum(s["wins"] for s in steps)
    assert env.stats() == st
    assert env.status() == 0


IDLE_AT = (0, 1, 777, 3071, 3072, 6143)    # first and last table, block and wave neighbours in between


class Idle:
    """6,144 tables of the run's start with empty-hand states at IDLE_AT, and the oracle's three iterations from them"""

    def __init__(self, oracle):
        T = 6144
        seed, base = WORLDS[T]
        ref = oracle.OracleEnv(T, seed=seed, gid_base=base)
        ref.reset()
        oracle.rollout_random_mt(ref, 5, THREADS)
        states = ref.state.reshape(T, cs.NFIELDS, cs.ROW).copy()
        table = cs.Table(*oracle.action_table())
        pick = np.flatnonzero(table.cards <= 17)[1:][:: 1500][:len(IDLE_AT)]
        empty = []
        for k in range(len(IDLE_AT)):
            role = k % 3
            _, s = cs.lead_exact(table, role, np.random.default_rng(30 + k), pick[k:k + 1])
            cs.check_consistent(s, table)
            # the actor's cards go to its history: every row sum still holds, only `done <=> an empty hand` does not
            h = s[0, cs.F_HAND0 + role, :15].copy()
            s[0, cs.F_HAND0 + role] = 0
            s[0, cs.F_HIST0 + role, :15] += h
            s[0, cs.F_TAKEN, :15] += h
            assert s[0, cs.F_META, cs.M_DONE] == 0 and s[0, cs.F_META, cs.M_ROLE] == role
            empty.append(s[0])
        states[list(IDLE_AT)] = np.stack(empty)
        self.T, self.seed, self.base = T, seed, base
        self.states = states
        ref.state[:] = states.reshape(-1)
        self.steps, _ = _steps(oracle, ref, 3)


_idle = []


@pytest.mark.parametrize("want_traj", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
def test_idle_iterations(pkg, oracle, iters, want_traj):
    if not _idle:
        _idle.append(Idle(oracle))
    w = _idle[0]
    at = list(IDLE_AT)
    steps = w.steps[:iters]
    # the oracle defines the case: an empty list, nothing applied, the record flagged 2 (no ply), in every iteration
    for s in steps:
        assert not s["sizes"][at].any() and np.all(s["traj"][at, 19] == 2)
        assert np.array_equal(s["state"].reshape(w.T, -1)[at], w.states.reshape(w.T, -1)[at])
    env = pkg.BatchedEnv(w.T, seed=w.seed, table_id_base=w.base, want_ids=False)
    env.state_import(torch.from_numpy(w.states.reshape(-1)))
    traj = torch.zeros((iters, w.T, 32), dtype=torch.uint8, device=_dev()) if want_traj else None
    env.rollout_random(iters, traj=traj)
    sizes, rows = _lists(env, "plain")
    state = _np(env.state)
    assert not sizes[at].any()
    assert np.array_equal(state.reshape(w.T, -1)[at], w.states.reshape(w.T, -1)[at])     # every iteration idled: rows unchanged
    got = {"sizes": sizes, "rows": rows, "state": state}
    want = {"sizes": steps[-1]["sizes"], "rows": steps[-1]["rows"], "state": steps[-1]["state"]}   # neighbours included
    if want_traj:
        got["traj"], want["traj"] = _np(traj), np.stack([s["traj"] for s in steps])
    assert cs.differences(got, want) == []
    st = env.stats()
    assert st["plies"] == (w.T - len(at)) * iters                                         # plies = iterations - idle
    assert st == dict(cs.run_stats([s["traj"] for s in steps]), legal_rows=sum(int(s["sizes"].sum()) for s in steps))
    assert env.status() == 0
