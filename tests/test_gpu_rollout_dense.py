"""GPU (-m gpu): the DENSE geometry of the fused rollout against the CPU oracle.

ddz_rollout_random picks 12-wave blocks (two per CU, several tables per wavefront) only without ids and when the grid
fills at least 5400 wavefronts, so the small batches of test_gpu_parity.py never reach it.  Here: 6,000 tables (1 table
per wavefront), 12,288 (2) and 65,536 (11), want_ids=False, launches of 1, 3, 64 and 300 iterations in sequence on the
same env (every table is dealt several times; a launch starts from whatever the one before stored), with and without
trajectory records.  After each launch, against OracleEnv stepped the same number of iterations: the whole packed state,
counts, the slab rows of the last iteration, the trajectory records, stats() and status() == 0.  Everything is bytes
and integers: every comparison is exact.

Trajectory records: the oracle writes them one lock-step iteration at a time on one thread, so every record of every
launch is compared at 6,000 tables and in the launches of 1 and 3 iterations of the larger batches; in their launches of
64 and 300 iterations the oracle runs all but the last iteration multi-threaded (rollout_random_mt) and the records of
the LAST iteration are compared (the state, stats and lists after it cover what the earlier ones did)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LAUNCHES = (1, 3, 64, 300)
THREADS = 16
F_HIST0, F_TAKEN, F_META = 3, 9, 10


@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


def _oracle_launch(oracle, ref, n, every_record):
    """n iterations of the oracle -> (list sizes, rows of the last pre-step states, records [k, T, 32] of the last k
    iterations, legal rows of the launch, episodes finished in the launch)"""
    rows_sum = episodes = 0
    if not every_record and n > 1:
        _, rows_sum, episodes = oracle.rollout_random_mt(ref, n - 1, THREADS)
    recs = []
    for _ in range(n if every_record else 1):
        roff, rrows, _ = ref.legal()
        sizes, rrows = np.diff(roff), rrows.copy()
        rows_sum += int(roff[-1])
        done, _, _, rtraj = ref.step(oracle.STEP_RANDOM, auto_reset=True, want_traj=True)
        episodes += int(done.sum())
        recs.append(rtraj)
    return sizes, rrows, np.stack(recs), rows_sum, episodes


@pytest.mark.parametrize("want_traj", [False, True])
@pytest.mark.parametrize("T,seed,base", [(6000, 41, 0), (12288, 42, 2 ** 40 + 7), (65536, 43, 123456789012)])
def test_dense_rollout_vs_oracle(pkg, oracle, T, seed, base, want_traj):
    env = pkg.BatchedEnv(T, seed=seed, table_id_base=base, want_ids=False)
    ref = oracle.OracleEnv(T, seed=seed, gid_base=base)
    env.reset(); ref.reset()
    assert np.array_equal(env.state.cpu().numpy(), ref.state)
    plies = rows_sum = episodes = 0
    for n in LAUNCHES:
        every = want_traj and (T == 6000 or n <= 3)
        sizes, rrows, rrecs, rs, ep = _oracle_launch(oracle, ref, n, every)
        traj = torch.zeros((n, T, 32), dtype=torch.uint8, device=_dev()) if want_traj else None
        env.rollout_random(n, traj=traj)
        counts = env.counts.cpu().numpy()
        print(f"T {T} launch of {n}: rows {int(counts.sum())} (oracle {int(sizes.sum())}), state bytes differing "
              f"{int((env.state.cpu().numpy() != ref.state).sum())}")
        assert np.array_equal(counts, sizes), n                          # lists of the last pre-step states
        mask = torch.arange(env.slab_stride, device=_dev())[None, :] < env.counts[:, None]
        assert np.array_equal(env.slab_rows()[mask].cpu().numpy(), rrows), n   # row-major gather == CSR order
        if want_traj:
            got = traj.cpu().numpy()
            assert np.array_equal(got[n - len(rrecs):], rrecs), n
        assert np.array_equal(env.state.cpu().numpy(), ref.state), n     # the whole packed state
        plies += T * n; rows_sum += rs; episodes += ep
        s = env.stats()                                                  # (accumulates until read: cumulative here)
        assert s["plies"] == plies and s["legal_rows"] == rows_sum and s["episodes"] == episodes, (n, s)
        assert s["lord_wins"] + s["up_wins"] + s["down_wins"] == s["episodes"]
        assert env.status() == 0
    assert episodes > 3 * T    # several deals per table


@pytest.mark.parametrize("want_traj", [False, True])
def test_dense_rollout_keeps_foreign_byte_15(pkg, want_traj):
    """A state whose history / taken rows carry a non-zero byte 15 (outside what the engine writes, inside the state
    format: the byte is the row's aux byte): the rollout never reads it and gives it back unchanged -- until the table is
    dealt again, which clears the whole row, as it always has.  Everything else equals the run from the clean state."""
    T = 6000
    a = pkg.BatchedEnv(T, seed=77, want_ids=False); b = pkg.BatchedEnv(T, seed=77, want_ids=False)
    a.reset(); a.rollout_random(37)
    clean = a.state_export()
    foreign = clean.clone().view(T, 11, 16)
    rng = np.random.default_rng(3)
    marks = torch.from_numpy(rng.integers(1, 256, (T, 4), dtype=np.uint8)).to(_dev())
    fields = [F_HIST0, F_HIST0 + 1, F_HIST0 + 2, F_TAKEN]
    for k, f in enumerate(fields):
        foreign[:, f, 15] = marks[:, k]
    b.state_import(foreign.view(-1))
    ep0 = a.state.view(T, 11, 16)[:, F_META, 8:12].clone()
    for n in (1, 3, 20):
        ta = torch.zeros((n, T, 32), dtype=torch.uint8, device=_dev()) if want_traj else None
        tb = torch.zeros_like(ta) if want_traj else None
        a.rollout_random(n, traj=ta); b.rollout_random(n, traj=tb)
        sa, sb = a.state.view(T, 11, 16).clone(), b.state.view(T, 11, 16).clone()
        same_episode = (sa[:, F_META, 8:12] == ep0).all(dim=1)
        assert int(same_episode.sum()) > 0    # (tables still in the episode the marks were put into)
        for k, f in enumerate(fields):
            expect = torch.where(same_episode, marks[:, k], torch.zeros_like(marks[:, k]))
            assert torch.equal(sb[:, f, 15], expect), (n, f)
            sb[:, f, 15] = sa[:, f, 15]
        assert torch.equal(sa, sb), n
        assert torch.equal(a.counts, b.counts)
        if want_traj:
            assert torch.equal(ta, tb)
    assert a.status() == 0 and b.status() == 0
