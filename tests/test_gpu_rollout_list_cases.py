"""GPU (-m gpu): k_rollout on the seam between the closed-form round of a list and its planner tail.  The states of
tests/rollout_list_cases.py (pinned against the CPU oracle in tests/test_rollout_list_cases_cpu.py: one table per case and
wanted list index, the episode forced so that the engine RNG draws that index) are imported and rolled out:
  dense     the sequence of tables repeated to 6,144 (distinct global ids, an episode searched per table): without ids the
            12-wave blocks of the headline variant (they run from 5,400 wavefronts on: tests/test_gpu_rollout_dense.py), one
            table per wavefront; with ids the 16-wave blocks at that size
  blocks16  the tables once, in 16-wave blocks
each with and without ids, with and without records, in launches of 1 and of 2 iterations (the second iteration plays, on the
registers the first one left, whatever follows the forced ply), and the cases holding both jokers once through the
joker-kicker library.  Against OracleEnv stepped the same way: counts, slab rows and ids of the last pre-step lists, every
record, the whole packed state, stats() and status() == 0.  Bytes and integers: everything is exact.  The oracle runs once
per set of tables (two iterations; the one-iteration launches are held to its first) and is never written."""
import numpy as np
import pytest
import torch

import constructed_states as cs
import rollout_list_cases as rc

pytestmark = pytest.mark.gpu
DENSE = 6144


@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


class World:
    def __init__(self, oracle, jk):
        self.oracle, self.jk = oracle, jk
        with oracle.variant(jk=jk):
            self.table = cs.Table(*oracle.action_table())
            self.cases = rc.build(oracle, self.table, both_jokers_only=jk)
        self.sets = {}

    def tables(self, layout):
        """(states, the oracle's two iterations from them)"""
        if layout not in self.sets:
            states, case, index, trials = rc.tables(self.cases, DENSE if layout == "dense" else None)
            assert (trials > 0).all()
            with self.oracle.variant(jk=self.jk):
                run, _ = cs.reference_run(self.oracle, states, 0, None, auto_reset=True, iters=2)
            # the forced ply is the wanted row of the wanted index, on every table
            assert np.array_equal(run[0]["traj"][:, :16], self.cases.rows[self.cases.off[case] + index])
            self.sets[layout] = (states, run)
        return self.sets[layout]


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle, False)


@pytest.fixture(scope="module")
def world_jk(oracle):
    return World(oracle, True)


def _np(x):
    return x.cpu().numpy()


def _case(w, pkg, layout, want_ids, want_traj, iters):
    states, run = w.tables(layout)
    run = run[:iters]
    T = len(states)
    env = pkg.BatchedEnv(T, seed=cs.SEED, device=_dev(), table_id_base=cs.GID_BASE, native_joker_kickers=w.jk, want_ids=want_ids)
    env.state_import(torch.from_numpy(states.reshape(-1)))
    traj = torch.zeros((iters, T, 32), dtype=torch.uint8, device=_dev()) if want_traj else None
    env.rollout_random(iters, traj=traj)
    S = env.slab_stride
    take = (torch.arange(S, device=_dev())[None, :] < env.counts[:, None]).reshape(-1)
    last = run[-1]
    got = {"off": np.concatenate([[0], np.cumsum(_np(env.counts).astype(np.int64))]).astype(np.int32),
           "rows": _np(env.rows[:T * S][take]), "state": _np(env.state)}
    want = {"off": last["off"], "rows": last["rows"], "state": last["state"]}
    if want_ids:
        got["ids"], want["ids"] = _np(env.ids[:T * S][take]), last["ids"]
    if want_traj:
        got["traj"], want["traj"] = _np(traj), np.stack([r["traj"] for r in run])
    assert cs.differences(got, want) == [], (layout, want_ids, want_traj, iters)
    st = dict(cs.run_stats([r["traj"] for r in run]), legal_rows=sum(int(r["off"][-1]) for r in run))
    assert env.stats() == st
    assert env.status() == 0


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("want_traj", [False, True])
@pytest.mark.parametrize("want_ids", [False, True])
@pytest.mark.parametrize("layout", ["dense", "blocks16"])
def test_rollout_on_the_list_cases(pkg, world, layout, want_ids, want_traj, iters):
    _case(world, pkg, layout, want_ids, want_traj, iters)


def test_rollout_on_the_joker_cases_with_joker_kickers(pkg, world_jk):
    _case(world_jk, pkg, "blocks16", True, True, 2)
