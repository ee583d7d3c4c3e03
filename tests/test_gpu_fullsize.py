"""GPU (-m gpu): BASELINE.json configs at their full sizes -- the policy-driven loop of configs[2] (65,536 tables:
observe -> per-action values -> select -> step), the same on the last shard of configs[4] (rank 7 of 8: table ids
7 * 65,536 ...), and configs[3] (rule farmers) -- through size-independent invariants, plus a 2,048-table slice of each
loop compared bit-exactly with the oracle."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NA = 13527
T_FULL = 65536
DECK = np.array([4] * 13 + [1, 1])


@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


def _q_for(gids, it, stride):
    """deterministic per-(global table, iteration) action values, identical whatever the shard: f32 [n, stride]"""
    g = torch.Generator(device="cpu").manual_seed(1000 + it)
    base = torch.rand(stride, generator=g)
    j = torch.arange(stride, dtype=torch.float64)
    return ((base.double()[None, :] + ((gids.double()[:, None] * 0.6180339887 + j[None, :] * 0.7548776662) % 1.0)) % 1.0).float()


def _check_invariants(pkg, env, it):
    T = env.T
    st = env.state.view(T, 11, 16).permute(1, 0, 2).cpu().numpy().astype(np.int64)
    hands = st[0:3, :, :15]
    assert np.array_equal(hands.sum(0) + st[9, :, :15], np.tile(DECK, (T, 1)))     # card conservation
    assert np.array_equal(st[3:6, :, :15].sum(0), st[9, :, :15])                   # taken = sum of histories
    assert np.array_equal(hands.sum(2), st[0:3, :, 15])                            # left = |hand|
    assert (st[10, :, 1] == 0).all() and (st[10, :, 6] == 1).all()                # auto-reset: every table live
    role = st[10, :, 0]
    ar = np.arange(T)
    own = hands[role, ar]
    # face (EnvCooperationSimplify, envi.py:202-217): plane 0 = thermometer of the actor's hand, plane 1 of `taken`,
    # planes 4,5 = the two probability planes: per rank they share out exactly the unseen cards (spec v1)
    face = env.observe(3)
    f = face.cpu().numpy()
    assert np.array_equal(f[:, 0].sum(2), own) and np.array_equal(f[:, 1].sum(2), st[9, :, :15])
    assert np.array_equal(f[:, 2].sum(2), st[6 + (role + 2) % 3, ar, :15])         # recent handout of (role-1)%3
    unseen = np.tile(DECK, (T, 1)) - own - st[9, :, :15]
    assert np.allclose((f[:, 4] + f[:, 5]).sum(2), unseen, atol=1e-5)
    n1, n2 = st[(role + 1) % 3, ar, 15], st[(role + 2) % 3, ar, 15]
    assert np.allclose(f[:, 4].sum((1, 2)) * (n1 + n2), unseen.sum(1) * n1, rtol=1e-5, atol=1e-4)
    # legal lists (slab) vs the dense mask: popcount(mask) = list size; rows fit the hand; ids ascending
    counts = env.counts.cpu().numpy().astype(np.int64)
    mask = env.legal_mask()
    bits = (mask.view(torch.int32).unsqueeze(-1) >> torch.arange(32, device=mask.device, dtype=torch.int32)) & 1
    assert np.array_equal(bits.sum((1, 2)).cpu().numpy(), counts)
    assert (counts >= 1).all() and counts.max() <= 497
    ids = env.slab_ids()
    valid = torch.arange(env.slab_stride, device=ids.device)[None, :] < env.counts[:, None]
    asc = (ids[:, 1:] > ids[:, :-1]) | ~valid[:, 1:]
    assert bool(asc.all())
    picked = bits.view(T, -1)[:, :NA].gather(1, ids.clamp(0, NA - 1).long()) == 1
    assert bool((picked | ~valid).all())                                           # every listed id is set in the mask
    rows = env.slab_rows()[:, :, :15].to(torch.int16)
    fits = (rows <= torch.from_numpy(own).to(rows.device, torch.int16)[:, None, :]).all(2)
    assert bool((fits | ~valid).all())                                             # counter_subset (utils.py:16-22)
    return st


@pytest.mark.parametrize("base", [0, 7 * T_FULL], ids=["configs2_tables_0..65535", "configs4_rank7_of_8"])
def test_policy_loop_full_size_with_oracle_slice(pkg, oracle, base):
    """configs[2] / one shard of configs[4]: 60 iterations of observe -> q -> select_slab -> step_slab(CHOICE) at
    65,536 tables; invariants on all tables, and tables [4096, 6144) of the shard bit-exact against the oracle."""
    T, iters, lo, n = T_FULL, 60, 4096, 2048
    env = pkg.BatchedEnv(T, seed=2026, device=_dev(), table_id_base=base)
    ref = oracle.OracleEnv(n, seed=2026, gid_base=base + lo)
    env.reset(); ref.reset()
    env.legal_slab()
    gids = torch.arange(base, base + T)
    stride = env.slab_stride
    face = torch.empty((T, 6, 15, 4), dtype=torch.float32, device=_dev())
    assert np.array_equal(env.state.view(T, -1)[lo:lo + n].cpu().numpy().reshape(-1), ref.state)
    for it in range(iters):
        q = _q_for(gids, it, stride).to(_dev())
        env.observe(3, out=face)
        choice = env.select_slab(q)
        # the oracle on the slice: same values in CSR order
        off, _, _ = ref.legal()
        cnt = np.diff(off)
        assert np.array_equal(env.counts[lo:lo + n].cpu().numpy(), cnt)
        qs = q[lo:lo + n].cpu().numpy()
        qcsr = np.concatenate([qs[t, :cnt[t]] for t in range(n)])
        rchoice = ref.select(qcsr)
        assert np.array_equal(choice[lo:lo + n].cpu().numpy(), rchoice)
        if it % 10 == 0:
            assert np.array_equal(face[lo:lo + n].cpu().numpy().view(np.uint32), ref.observe(3).view(np.uint32))
        done, rew, ill = env.step_slab(choice, pkg.STEP_CHOICE, auto_reset=True)
        rdone, rrew, rill, _ = ref.step(oracle.STEP_CHOICE, rchoice, auto_reset=True)
        assert not bool(ill.any())
        assert np.array_equal(done[lo:lo + n].cpu().numpy(), rdone) and np.array_equal(rew[lo:lo + n].cpu().numpy(), rrew)
        assert np.array_equal(env.state.view(T, -1)[lo:lo + n].cpu().numpy().reshape(-1), ref.state), it
        if it % 20 == 19:
            _check_invariants(pkg, env, it)
    assert env.status() == 0
    s = env.stats()
    assert s["plies"] == T * iters and s["episodes"] > 0


def test_rule_opponent_full_size_with_oracle_slice(pkg, oracle):
    """configs[3]: 65,536 tables, farmers = rule agent, lord = engine RNG, 45 iterations; invariants on all tables, the
    rule agent's choices and the states of tables [1024, 1536) bit-exact against the oracle; farmers win most games."""
    T, iters, lo, n = T_FULL, 45, 1024, 512
    env = pkg.BatchedEnv(T, seed=99, device=_dev())
    ref = oracle.OracleEnv(n, seed=99, gid_base=lo)
    env.reset(); ref.reset()
    env.legal_slab()
    for it in range(iters):
        ids = env.auto_choose(0b101)
        rids = ref.auto_choose(0b101)
        assert np.array_equal(ids[lo:lo + n].cpu().numpy(), rids), it
        role = env.role
        assert bool(((ids >= 0) == (role != 1)).all())          # exactly the farmers' tables carry a choice
        done, rew, ill = env.step_slab(ids, pkg.STEP_IDS, auto_reset=True)
        ref.legal()
        rdone, rrew, _, _ = ref.step(oracle.STEP_IDS, rids, auto_reset=True)
        assert not bool(ill.any())
        assert np.array_equal(env.state.view(T, -1)[lo:lo + n].cpu().numpy().reshape(-1), ref.state), it
        if it % 15 == 14:
            _check_invariants(pkg, env, it)
    assert env.status() == 0
    s = env.stats()
    assert s["episodes"] > T // 4 and s["up_wins"] + s["down_wins"] > 2 * s["lord_wins"]


def test_q_features_and_q_csr_equal_the_torch_statement_and_the_literal_network(pkg):
    """The first layer of the ragged Q forward by ddz_q_features (FactorisedQ.tables) == the same stage in plain torch ops,
    and FactorisedQ.q_csr over the CSR rows of the slab lists (the training path, ragged_q) == the literal nn.Conv2d
    evaluation of net.py:81-102 on a sample of rows.  Floating point, fp32: tolerance 1e-5 absolute (summation order is
    the only difference)."""
    import importlib
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    for T, variant in ((3001, 3), (517, 2), (64, 0), (1000, 1)):
        P = pkg.FACE_PLANES[variant]
        torch.manual_seed(variant)
        net = glue.QNet(P).to(_dev()).eval()
        env = pkg.BatchedEnv(T, seed=5 + variant, device=_dev())
        env.reset()
        env.rollout_random(9 if variant else 0)        # variant 0: fresh deals, 20-card leads (long lists)
        env.legal_slab()
        face = env.observe(variant)
        fq = glue.FactorisedQ(net, chunk_tables=1024)
        U = fq.tables(face)                            # first layer by ddz_q_features (one pass over `face`)
        U_torch = fq.tables(face, fused=False)         # ... and the same stage in plain torch ops
        assert torch.allclose(U, U_torch, rtol=1e-5, atol=1e-5), float((U - U_torch).abs().max())
        off, rows, _ = env.slab_to_csr(rows_per_table=512)
        qc = fq.q_csr(U, rows, off)
        n = int(off[-1].item())
        counts = env.counts.long()
        assert int(counts.sum()) == n
        # literal evaluation on every 7th row -- on the CPU (MIOpen would tune a convolution for every new batch size)
        seg = torch.repeat_interleave(torch.arange(T, device=_dev()), counts)
        pick = torch.arange(0, n, 7, device=_dev())
        acts = pkg.rows_to_onehot(rows[:n][pick])
        with torch.no_grad():
            want = copy.deepcopy(net).cpu()(face[seg[pick]].cpu(), acts.cpu())[:, 0]
        assert float((qc[:n][pick].cpu() - want).abs().max()) < 1e-5
        assert env.status() == 0


def test_policy_loop_with_the_q_network_full_size_with_oracle_slice(pkg, oracle):
    """configs[2] as SURVEY 8(d) defines it: 65,536 tables, EnvCooperationSimplify planes, NetCooperationSimplify
    randomly initialised (torch.manual_seed(0), eval), greedy arg-max per table -- dqn_glue.PolicyLoop, nothing on the
    host between the iterations.  Tables [4096, 6144) are stepped by the oracle from the SAME q values (copied out of the
    loop): choices, done / r and full states bit-exact every iteration; the q values themselves against the literal
    network on the slice (fp32, 1e-5); invariants on all tables."""
    import importlib
    glue = importlib.import_module("doudizhu-rl_amd.dqn_glue")
    T, iters, lo, n = T_FULL, 12, 4096, 2048
    torch.manual_seed(0)
    net = glue.QNet(6).to(_dev()).eval()
    net_cpu = copy.deepcopy(net).cpu()          # the literal network runs on the CPU (no MIOpen tuning per batch size)
    env = pkg.BatchedEnv(T, seed=77, device=_dev())
    ref = oracle.OracleEnv(n, seed=77, gid_base=lo)
    env.reset(); ref.reset()
    loop = glue.PolicyLoop(env, net, face_variant=3, epsilon=0.0)
    for it in range(iters):
        q = loop.q_values()                                      # [T, stride]; the loop's step() recomputes the same
        off, rrows, _ = ref.legal()
        cnt = np.diff(off)
        assert np.array_equal(env.counts[lo:lo + n].cpu().numpy(), cnt)
        qs = q[lo:lo + n].cpu().numpy()
        qcsr = np.concatenate([qs[t, :cnt[t]] for t in range(n)])
        rchoice = ref.select(qcsr)
        if it % 4 == 0:                                          # the values: literal network on the slice's rows
            seg = torch.from_numpy(np.repeat(np.arange(n), cnt))
            acts = (torch.from_numpy(rrows[:, :15].astype(np.float32))[:, :, None] > torch.arange(4)[None, None, :]).float()
            with torch.no_grad():
                want = net_cpu(loop.face[lo:lo + n].cpu()[seg], acts)[:, 0]
            assert float((torch.from_numpy(qcsr) - want).abs().max()) < 1e-5
            assert np.array_equal(loop.face[lo:lo + n].cpu().numpy().view(np.uint32), ref.observe(3).view(np.uint32))
        done, rew, ill = loop.step()
        assert np.array_equal(loop.choice[lo:lo + n].cpu().numpy(), rchoice), it
        rdone, rrew, rill, _ = ref.step(oracle.STEP_CHOICE, rchoice, auto_reset=True)
        assert not bool(ill.any())
        assert np.array_equal(done[lo:lo + n].cpu().numpy(), rdone) and np.array_equal(rew[lo:lo + n].cpu().numpy(), rrew)
        assert np.array_equal(env.state.view(T, -1)[lo:lo + n].cpu().numpy().reshape(-1), ref.state), it
    _check_invariants(pkg, env, iters)
    assert env.status() == 0 and env.stats()["plies"] == T * iters
