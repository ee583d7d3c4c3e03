"""GPU (-m gpu): the HIP path, called through the C ABI via the host mirror, against
(1) the committed golden fixtures from the reference's rules and (2) the CPU oracle on the
same seeded inputs.  Integer/byte/index work: every comparison is bit-exact; the two f32
probability planes of `face` are a single IEEE division and are compared bit-exactly too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NA = 13527


@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("doudizhu-rl_amd")


def _dev():
    return torch.device("cuda:0")


def test_classify_every_action_row(pkg, golden):
    """device classify() == CardGroup.to_cardgroup (card.py:327-335) on all 13,527 rows."""
    import ctypes as C
    import importlib
    L = importlib.import_module("doudizhu-rl_amd._lib").lib()
    g = golden("action_table.npz")
    rows = torch.zeros((NA, 16), dtype=torch.int8)
    rows[:, :15] = torch.from_numpy(g["rows"])
    rows = rows.to(_dev())
    out = torch.zeros(NA, dtype=torch.int32, device=_dev())
    assert L.ddz_debug_classify(0, C.c_void_p(rows.data_ptr()), NA, C.c_void_p(out.data_ptr()), None) == 0
    info = out.cpu().numpy().astype(np.uint32)
    assert np.array_equal(info & 0xFF, g["tg_type"])
    assert np.array_equal((info >> 8) & 0xFF, g["tg_value"])
    assert np.array_equal((info >> 16) & 0xFF, g["tg_len"])


def test_classify_rejects_non_combos(pkg, oracle):
    import ctypes as C
    import importlib
    L = importlib.import_module("doudizhu-rl_amd._lib").lib()
    rng = np.random.default_rng(5)
    n = 20000
    rows = np.zeros((n, 16), np.int8)
    for k in range(n):
        m = rng.integers(1, 6)
        idx = rng.choice(15, m, replace=False)
        rows[k, idx] = rng.integers(1, 5, m)
        rows[k, 13:15] = np.minimum(rows[k, 13:15], 1)
    expect = np.array([oracle.lookup(r[:15]) for r in rows])
    d = torch.from_numpy(rows).to(_dev())
    out = torch.zeros(n, dtype=torch.int32, device=_dev())
    assert L.ddz_debug_classify(0, C.c_void_p(d.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == 0
    info = out.cpu().numpy().astype(np.uint32)
    assert np.array_equal(info == 0xFF, expect < 0)
    assert (expect >= 0).sum() > 500 and (expect < 0).sum() > 500
    _, oinfo = oracle.action_table()
    ok = expect >= 0
    assert np.array_equal(info[ok] & 0xFF, oinfo[expect[ok], 0])


def test_get_moves_golden_cases(pkg, golden):
    """r.get_moves drop-in vs the reference's get_mask_onehot60 outputs (G3)."""
    g = golden("legal_cases.npz")
    table = golden("action_table.npz")
    hands = torch.from_numpy(g["hands"]).to(_dev())
    lasts = torch.from_numpy(table["rows"][g["last_ids"]]).to(_dev())
    offsets, rows, ids = pkg.get_moves(hands, lasts)
    assert np.array_equal(offsets.cpu().numpy(), g["offsets"])
    assert np.array_equal(ids.cpu().numpy(), g["ids"].astype(np.int32))
    rows = rows.cpu().numpy()
    assert np.array_equal(rows[:, :15], table["rows"][g["ids"].astype(np.int64)])
    assert np.array_equal(rows[:, 15].astype(np.uint8), table["cat_range"][g["ids"].astype(np.int64)])


def test_get_moves_golden_sweep(pkg, golden):
    """G6 through ddz_get_moves: 4,000 random (hand, last) pairs vs the reference's get_mask_onehot60 outputs."""
    g = golden("legal_sweep.npz")
    table = golden("action_table.npz")
    hands = torch.from_numpy(g["hands"]).to(_dev())
    lasts = torch.from_numpy(table["rows"][g["last_ids"]]).to(_dev())
    offsets, rows, ids = pkg.get_moves(hands, lasts)
    assert np.array_equal(offsets.cpu().numpy(), g["offsets"])
    assert np.array_equal(ids.cpu().numpy(), g["ids"].astype(np.int32))
    assert np.array_equal(rows.cpu().numpy()[:, :15], table["rows"][g["ids"].astype(np.int64)])


def test_get_moves_rejects_bad_last(pkg):
    hands = torch.tensor([[4] * 13 + [1, 1]], dtype=torch.int8, device=_dev())
    lasts = torch.zeros((1, 15), dtype=torch.int8, device=_dev())
    lasts[0, 0] = 2; lasts[0, 1] = 1  # 3 3 4
    with pytest.raises(ValueError):
        pkg.get_moves(hands, lasts)


def test_episodes_golden(pkg, golden):
    """G4: seeded trajectories whose per-ply legal sets were checked against the reference
    mask when the fixture was generated; the device env must reproduce them bit for bit."""
    g = golden("episodes.npz")
    T, iters = int(g["n_tables"]), int(g["n_iters"])
    env = pkg.BatchedEnv(T, seed=int(g["seed"]), table_id_base=int(g["gid_base"]))
    env.reset()
    traj = torch.zeros((T, 32), dtype=torch.uint8, device=_dev())
    k = 0
    for it in range(iters):
        offsets, rows, ids = env.legal()
        off = offsets.cpu().numpy(); idv = ids.cpu().numpy()
        role = env.role.cpu().numpy()
        done, reward, illegal = env.step_random(auto_reset=True, traj=traj)
        done = done.cpu().numpy(); reward = reward.cpu().numpy()
        tr = traj.cpu().numpy()
        assert not illegal.any().item()
        for t in range(T):
            assert np.array_equal(idv[off[t]:off[t + 1]], g["ids"][g["offsets"][k]:g["offsets"][k + 1]])
            assert role[t] == g["role"][k]
            assert int(tr[t, 28:32].view(np.int32)[0]) == g["choice"][k]
            assert done[t] == g["done"][k] and reward[t] == g["reward"][k]
            k += 1
    assert np.array_equal(env.state.cpu().numpy(), g["final_state"])
    assert env.status() == 0


@pytest.mark.parametrize("T,iters,seed,base", [(1000, 130, 1, 0), (4096, 40, 2, 123456789012)])
def test_lockstep_vs_oracle(pkg, oracle, T, iters, seed, base):
    """every iteration: CSR offsets, rows, ids, done/reward and the full packed state."""
    env = pkg.BatchedEnv(T, seed=seed, table_id_base=base)
    ref = oracle.OracleEnv(T, seed=seed, gid_base=base)
    env.reset(); ref.reset()
    assert np.array_equal(env.state.cpu().numpy(), ref.state)
    traj = torch.zeros((T, 32), dtype=torch.uint8, device=_dev())
    for it in range(iters):
        offsets, rows, ids = env.legal()
        roff, rrows, rids = ref.legal()
        assert np.array_equal(offsets.cpu().numpy(), roff), it
        n = int(roff[-1])
        assert np.array_equal(ids[:n].cpu().numpy(), rids), it
        assert np.array_equal(rows[:n].cpu().numpy(), rrows), it
        done, reward, illegal = env.step_random(auto_reset=True, traj=traj)
        rdone, rreward, rillegal, rtraj = ref.step(oracle.STEP_RANDOM, auto_reset=True, want_traj=True)
        assert np.array_equal(done.cpu().numpy(), rdone)
        assert np.array_equal(reward.cpu().numpy(), rreward)
        assert np.array_equal(traj.cpu().numpy(), rtraj)
        assert np.array_equal(env.state.cpu().numpy(), ref.state), it
    assert env.status() == 0
    s = env.stats()
    assert s["plies"] == T * iters


@pytest.mark.parametrize("T,iters,seed,base", [(777, 140, 3, 0), (4096, 30, 8, 9876543210)])
def test_rollout_slabs_vs_oracle(pkg, oracle, T, iters, seed, base):
    """the fused rollout kernel (slab layout): after launches of 1..4 in-kernel iterations the
    list of every table, its ids, every iteration's trajectory record and the whole packed
    state equal the oracle's."""
    env = pkg.BatchedEnv(T, seed=seed, table_id_base=base)
    ref = oracle.OracleEnv(T, seed=seed, gid_base=base)
    env.reset(); ref.reset()
    it = 0
    while it < iters:
        n = 1 + (it % 4)
        traj = torch.zeros((n, T, 32), dtype=torch.uint8, device=_dev())
        rtrajs = []
        for _ in range(n):
            roff, rrows, rids = ref.legal()
            roff = roff.copy(); rrows = rrows.copy(); rids = rids.copy()
            _, _, _, rtraj = ref.step(oracle.STEP_RANDOM, auto_reset=True, want_traj=True)
            rtrajs.append(rtraj)
        env.rollout_random(n, traj=traj)
        counts = env.counts.cpu().numpy()
        assert np.array_equal(counts, np.diff(roff)), it      # lists of the last pre-step state
        slab = env.slab_rows().cpu().numpy(); sids = env.slab_ids().cpu().numpy()
        mask = np.arange(env.slab_stride)[None, :] < counts[:, None]
        assert np.array_equal(slab[mask], rrows), it           # row-major gather == CSR order
        assert np.array_equal(sids[mask], rids), it
        assert np.array_equal(traj.cpu().numpy(), np.stack(rtrajs)), it
        assert np.array_equal(env.state.cpu().numpy(), ref.state), it
        it += n
    assert env.status() == 0
    s = env.stats()
    assert s["plies"] == T * it and s["legal_rows"] > 0
    assert s["lord_wins"] + s["up_wins"] + s["down_wins"] == s["episodes"]
    assert min(s["lord_wins"], s["up_wins"], s["down_wins"]) > 0 or T < 100


def test_win_counts_match_trajectories(pkg):
    """stats (Game.compete's per-role wins, game.py:258-290) against the trajectory records,
    for both rollout variants"""
    T, n = 2000, 150
    for variant in ("slab", "csr"):
        env = pkg.BatchedEnv(T, seed=17)
        env.reset()
        traj = torch.zeros((n, T, 32), dtype=torch.uint8, device=_dev())
        (env.rollout_random if variant == "slab" else env.rollout_random_csr)(n, traj=traj)
        tr = traj.cpu().numpy()
        done, role = tr[..., 17] == 1, tr[..., 16]
        s = env.stats()
        assert s["episodes"] == done.sum() > 3000
        assert [s["up_wins"], s["lord_wins"], s["down_wins"]] == [int((done & (role == r)).sum()) for r in range(3)]
        assert s["plies"] == T * n


@pytest.mark.parametrize("T", [1, 7, 9, 513])
def test_ragged_table_counts(pkg, oracle, T):
    """table counts that do not fill a block / a wave group: CSR path and rollout path"""
    env = pkg.BatchedEnv(T, seed=6, table_id_base=2 ** 40 + 5)
    env2 = pkg.BatchedEnv(T, seed=6, table_id_base=2 ** 40 + 5)
    ref = oracle.OracleEnv(T, seed=6, gid_base=2 ** 40 + 5)
    env.reset(); env2.reset(); ref.reset()
    for it in range(70):
        offsets, rows, ids = env.legal()
        roff, rrows, rids = ref.legal()
        n = int(roff[-1])
        assert np.array_equal(offsets.cpu().numpy(), roff)
        assert np.array_equal(rows[:n].cpu().numpy(), rrows) and np.array_equal(ids[:n].cpu().numpy(), rids)
        env.step_random(); ref.step(oracle.STEP_RANDOM)
        assert np.array_equal(env.state.cpu().numpy(), ref.state)
    env2.rollout_random(70)
    assert np.array_equal(env2.state.cpu().numpy(), ref.state)
    assert env.status() == 0 and env2.status() == 0


@pytest.mark.parametrize("batch,want_ids", [(None, True), (0, True), (7, True), (1, True), (64, False)])
def test_rollout_csr_equals_slab_rollout(pkg, oracle, batch, want_ids):
    """the CSR-list variants of the fused rollout -- staged batches compacted by two launches per batch (the default; batch
    sizes that divide the iteration count, that do not, and that exceed it), and one launch per iteration (batch 0): same
    trajectories and states as the slab rollout, and the lists left in offsets / rows / ids are byte for byte the oracle's
    CSR lists of the last iteration's pre-step states"""
    T, n = 1500, 60
    a = pkg.BatchedEnv(T, seed=31, want_ids=want_ids); b = pkg.BatchedEnv(T, seed=31, want_ids=want_ids); ref = oracle.OracleEnv(T, seed=31)
    a.reset(); b.reset(); ref.reset()
    ta = torch.zeros((n, T, 32), dtype=torch.uint8, device=_dev()); tb = torch.zeros_like(ta)
    a.rollout_random(n, traj=ta)
    b.rollout_random_csr(n, traj=tb, batch=batch)
    assert torch.equal(ta, tb) and torch.equal(a.state, b.state)
    for _ in range(n - 1):
        ref.legal(); ref.step(oracle.STEP_RANDOM)
    roff, rrows, rids = ref.legal()
    ref.step(oracle.STEP_RANDOM)
    m = int(roff[-1])
    assert np.array_equal(b.offsets.cpu().numpy(), roff)
    assert np.array_equal(b.rows[:m].cpu().numpy(), rrows) and (not want_ids or np.array_equal(b.ids[:m].cpu().numpy(), rids))
    assert np.array_equal(b.state.cpu().numpy(), ref.state) and b.status() == 0
    # a second call continues from the new states (a staging buffer that is reused, frozen tables included)
    b.rollout_random_csr(5, batch=batch); a.rollout_random(5)
    assert torch.equal(a.state, b.state)


def test_no_auto_reset_freezes_tables(pkg, oracle):
    T = 512
    env = pkg.BatchedEnv(T, seed=9)
    ref = oracle.OracleEnv(T, seed=9)
    env.reset(); ref.reset()
    for it in range(170):  # longer than any episode (<= 162 plies)
        env.legal(); ref.legal()
        done, reward, _ = env.step_random(auto_reset=False)
        rdone, rreward, _, _ = ref.step(oracle.STEP_RANDOM, auto_reset=False)
        assert np.array_equal(done.cpu().numpy(), rdone)
        assert np.array_equal(reward.cpu().numpy(), rreward)
    assert done.all().item()
    assert np.array_equal(env.state.cpu().numpy(), ref.state)
    offsets, _, _ = env.legal()
    assert int(offsets[-1].item()) == 0  # frozen tables have empty lists
    mask = torch.zeros(T, dtype=torch.uint8); mask[::2] = 1
    env.reset(mask); ref.reset(mask.numpy())
    assert np.array_equal(env.state.cpu().numpy(), ref.state)
    offsets, _, _ = env.legal(); roff, _, _ = ref.legal()
    assert np.array_equal(offsets.cpu().numpy(), roff)


def test_step_choice_rows_and_illegal(pkg, oracle):
    T = 256
    env = pkg.BatchedEnv(T, seed=4)
    ref = oracle.OracleEnv(T, seed=4)
    env.reset(); ref.reset()
    rng = np.random.default_rng(0)
    for it in range(60):
        offsets, rows, ids = env.legal()
        roff, rrows, _ = ref.legal()
        A = np.diff(roff)
        if it % 2 == 0:
            choice = (rng.integers(0, 1 << 30, T) % np.maximum(A, 1)).astype(np.int32)
            choice[it % T] = A[it % T] + 3          # out of range -> illegal
            choice[(it + 7) % T] = -1
            done, reward, illegal = env.step(torch.from_numpy(choice), pkg.STEP_CHOICE, auto_reset=True)
            rdone, rreward, rillegal, _ = ref.step(oracle.STEP_CHOICE, choice, auto_reset=True)
        else:
            pick = roff[:-1] + (rng.integers(0, 1 << 30, T) % np.maximum(A, 1))
            sel = rrows[pick].copy()
            sel[:, 15] = 0                            # callers need not know the category byte
            sel[it % T, :15] = 0; sel[it % T, 0] = 3; sel[it % T, 1] = 1; sel[it % T, 2] = 1  # no combo
            done, reward, illegal = env.step(torch.from_numpy(sel), pkg.STEP_ROWS, auto_reset=True)
            rdone, rreward, rillegal, _ = ref.step(oracle.STEP_ROWS, sel, auto_reset=True)
        assert np.array_equal(illegal.cpu().numpy(), rillegal) and rillegal.sum() >= 1
        assert np.array_equal(done.cpu().numpy(), rdone)
        assert np.array_equal(reward.cpu().numpy(), rreward)
        assert np.array_equal(env.state.cpu().numpy(), ref.state)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_observe_vs_oracle(pkg, oracle, variant):
    T = 777
    env = pkg.BatchedEnv(T, seed=21)
    ref = oracle.OracleEnv(T, seed=21)
    env.reset(); ref.reset()
    for it in range(23):
        env.legal(); ref.legal()
        env.step_random(); ref.step(oracle.STEP_RANDOM)
    face = env.observe(variant).cpu().numpy()
    want = ref.observe(variant)
    assert face.shape == want.shape == (T, pkg.FACE_PLANES[variant], 15, 4)
    assert np.array_equal(face.view(np.uint32), want.view(np.uint32))  # bit-exact, prob planes too


def test_rows_to_onehot_golden(pkg, golden):
    bits = np.unpackbits(golden("thermo.npz")["bits"], axis=1)[:, :60]
    rows = torch.zeros((NA, 16), dtype=torch.int8)
    rows[:, :15] = torch.from_numpy(golden("action_table.npz")["rows"])
    oh = pkg.rows_to_onehot(rows.to(_dev())).cpu().numpy()
    assert oh.shape == (NA, 15, 4)
    assert np.array_equal(oh.reshape(NA, 60).astype(np.uint8), bits)


def test_full_deck_hand_lists_every_action(pkg):
    hands = torch.tensor([[4] * 13 + [1, 1]], dtype=torch.int8, device=_dev())
    lasts = torch.zeros((1, 15), dtype=torch.int8, device=_dev())
    offsets, rows, ids = pkg.get_moves(hands, lasts)
    assert offsets.tolist() == [0, NA - 1]
    assert torch.equal(ids.cpu(), torch.arange(1, NA, dtype=torch.int32))


@pytest.mark.parametrize("T", [4096, 65536, 524288])
def test_full_size_properties(pkg, T):
    """BASELINE sizes (524,288 = all tables of configs[4] on one GPU): size-independent invariants after a seeded
    random-policy rollout."""
    iters = 150
    env = pkg.BatchedEnv(T, seed=77)
    env.reset()
    env.rollout_random(iters)
    offsets, rows, ids = env.legal()
    assert env.status() == 0
    s = env.stats()
    assert s["plies"] == T * iters
    assert 0.8 * T * iters / 66 < s["episodes"] < 1.25 * T * iters / 60   # ~65 plies per episode
    assert 0 < s["lord_wins"] < s["episodes"]
    st = env.state.view(T, 11, 16).permute(1, 0, 2).cpu().numpy().astype(np.int64)
    deck = np.array([4] * 13 + [1, 1])
    hands = st[0:3, :, :15]
    assert np.array_equal(hands.sum(0) + st[9, :, :15], np.tile(deck, (T, 1)))     # conservation
    assert np.array_equal(st[3:6, :, :15].sum(0), st[9, :, :15])                   # taken = sum history
    assert np.array_equal(hands.sum(2), st[0:3, :, 15])                            # left = |hand|
    assert (st[0:3, :, 15] > 0).all() and (st[10, :, 1] == 0).all()               # auto-reset: none done
    off = offsets.cpu().numpy().astype(np.int64)
    assert off[0] == 0 and (np.diff(off) >= 1).all()
    total = off[-1]
    idv = ids[:total].cpu().numpy(); rw = rows[:total].cpu().numpy()
    seg = np.repeat(np.arange(T), np.diff(off))
    role = st[10, :, 0]
    own = hands[role, np.arange(T)]                                                # [T,15]
    assert (rw[:, :15] <= own[seg]).all()                                          # counter_subset
    inc = np.diff(idv) > 0
    same = seg[1:] == seg[:-1]
    assert inc[same].all()                                                         # ascending ids
    assert (idv >= 0).all() and (idv < NA).all()


@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
def test_select_matches_argmax_and_oracle(pkg, oracle, eps):
    """greedy / epsilon-greedy selection (dqn.py:50-71) over the CSR list, then a CHOICE step."""
    T = 3000
    env = pkg.BatchedEnv(T, seed=12)
    ref = oracle.OracleEnv(T, seed=12)
    env.reset(); ref.reset()
    g = torch.Generator().manual_seed(1)
    explored = 0
    for it in range(25):
        offsets, rows, ids = env.legal()
        roff, _, _ = ref.legal()
        n = int(roff[-1])
        q = torch.randint(-3, 4, (n,), generator=g).float()      # many ties: argmax must take the first
        choice = env.select(q.to(_dev()), eps)
        want = ref.select(q.numpy(), eps)
        assert np.array_equal(choice.cpu().numpy(), want)
        if eps == 0.0:
            seg = np.repeat(np.arange(T), np.diff(roff))
            first = np.array([int(torch.argmax(q[roff[t]:roff[t + 1]])) for t in range(0, T, 37)])
            assert np.array_equal(want[::37], first)              # torch.argmax semantics (dqn.py:60)
        else:
            greedy = ref.select(q.numpy(), 0.0)
            explored += int((want != greedy).sum())
        env.step(choice, pkg.STEP_CHOICE); ref.step(oracle.STEP_CHOICE, want)
        assert np.array_equal(env.state.cpu().numpy(), ref.state)
    if eps > 0:
        assert explored > 0


def test_select_long_lists_ties_and_nans(pkg, oracle):
    """k_select reads a list with 16 lanes and merges them: on lead states with long lists (up to ~130 moves), values
    from a 3-level set (ties across lanes) and sprinkled NaNs, CSR and slab forms pick what the sequential scan of
    dqn.py:60's arg-max does (first maximum; a NaN never replaces, a NaN in entry 0 stays)."""
    T = 2048
    env = pkg.BatchedEnv(T, seed=8, device=_dev())
    ref = oracle.OracleEnv(T, seed=8)
    env.reset(); ref.reset()                       # every table: the lord leads with 20 cards
    g = torch.Generator().manual_seed(5)
    for it in range(6):
        offsets, _, _ = env.legal()
        roff, _, _ = ref.legal()
        n = int(roff[-1])
        cnt = np.diff(roff)
        if it == 0:
            assert cnt.max() > 64 and cnt.min() > 16
        q = torch.randint(0, 3, (n,), generator=g).float()
        q[torch.rand(n, generator=g) < 0.05] = float("nan")
        q[torch.from_numpy(roff[:-1][::5].astype(np.int64))] = float("nan")   # entry 0 of every fifth table
        want = ref.select(q.numpy(), 0.0)
        seq = np.zeros(T, np.int32)
        qn = q.numpy()
        for t in range(T):
            b = 0
            for j in range(1, cnt[t]):
                if qn[roff[t] + j] > qn[roff[t] + b]:
                    b = j
            seq[t] = b
        assert np.array_equal(want, seq)
        assert np.array_equal(env.select(q.to(_dev())).cpu().numpy(), want)
        counts, _, _ = env.legal_slab()
        qs = torch.full((T, env.slab_stride), 7.0)
        for t in range(T):
            qs[t, :cnt[t]] = q[roff[t]:roff[t + 1]]
        assert np.array_equal(env.select_slab(qs.to(_dev())).cpu().numpy(), want)
        env.step_slab(torch.from_numpy(want), pkg.STEP_CHOICE, auto_reset=False)
        ref.step(oracle.STEP_CHOICE, want, auto_reset=False)
        env.reset(); ref.reset()                   # next episode: new 20-card leads


@pytest.mark.parametrize("eps,variant,want_ids,tpw", [(0.0, 3, True, 1), (0.3, 2, False, 1), (0.0, 0, True, 7), (1.0, 1, True, 16),
                                                      (0.2, 3, False, 37), (0.0, 2, True, 20)])
def test_policy_step_slab_equals_separate_calls(pkg, eps, variant, want_ids, tpw):
    """ddz_policy_step_slab (select + step + new lists + face in ONE launch) == select_slab -> step_slab -> observe:
    choices, done / r / illegal, trajectory records, states, lists and `face` bit-identical, every iteration; one table
    per wave (wave 0 of a block runs the block's lane-parallel phases) and several chunkings of 16-table chunks (the
    fused kernel writes `face` before the lists in half of its waves and after them in the other half)."""
    T = 3000
    a = pkg.BatchedEnv(T, seed=41, device=_dev(), want_ids=want_ids, _debug_tables_per_wave=tpw)  # ddz_debug_set_geometry
    b = pkg.BatchedEnv(T, seed=41, device=_dev(), want_ids=want_ids)
    a.reset(); b.reset()
    a.legal_slab(); b.legal_slab()
    g = torch.Generator().manual_seed(9)
    P = pkg.FACE_PLANES[variant]
    for it in range(70):
        q = torch.randint(-2, 3, (T, a.slab_stride), generator=g).float().to(_dev())   # ties on purpose
        auto = it % 6 != 5
        ta = torch.zeros((T, 32), dtype=torch.uint8, device=_dev())
        tb = torch.zeros((T, 32), dtype=torch.uint8, device=_dev())
        ca = torch.empty(T, dtype=torch.int32, device=_dev())
        with_face = it % 4 != 3   # every fourth iteration without a face output: that form of the fused launch hands
        da, ra, ia, fa = a.policy_step_slab(q, eps, face_variant=variant if with_face else None, choice_out=ca,   # deals and
                                            auto_reset=auto, traj=ta)                             # lists out by the block work list
        cb = b.select_slab(q, eps)
        db, rb, ib = b.step_slab(cb, pkg.STEP_CHOICE, auto_reset=auto, traj=tb)
        fb = b.observe(variant)
        assert torch.equal(ca, cb) and torch.equal(da, db) and torch.equal(ra, rb) and torch.equal(ia, ib), it
        assert torch.equal(ta, tb) and torch.equal(a.state, b.state) and torch.equal(a.counts, b.counts), it
        if with_face:
            assert fa.shape == (T, P, 15, 4) and torch.equal(fa.view(torch.int32), fb.view(torch.int32)), it
        else:
            assert fa is None
        m = torch.arange(a.slab_stride, device=_dev())[None, :] < a.counts[:, None]
        assert torch.equal(a.slab_rows()[m], b.slab_rows()[m])
        if want_ids:
            assert torch.equal(a.slab_ids()[m], b.slab_ids()[m])
        if it % 12 == 11:
            mk = a.field(10)[:, 1] != 0
            a.reset(mask=mk); b.reset(mask=mk)
            a.legal_slab(); b.legal_slab()
    assert a.status() == 0 and a.stats() == b.stats()


def test_get_moves_slab_golden_and_csr(pkg, golden):
    """ddz_get_moves_slab (one launch, slab layout) == the reference's legal sets (G3, G6) == ddz_get_moves (CSR);
    a `last` that is no combo and a hand whose list does not fit are reported, not written."""
    for name in ("legal_cases.npz", "legal_sweep.npz"):
        g = golden(name)
        table = golden("action_table.npz")["rows"]
        hands = g["hands"].astype(np.int8)
        lasts = table[g["last_ids"]].astype(np.int8)
        small = hands.sum(1) <= 20
        h, l = torch.from_numpy(hands[small]).to(_dev()), torch.from_numpy(lasts[small]).to(_dev())
        counts, rows, ids, status = pkg.get_moves_slab(h, l)
        off, crow, cid = pkg.get_moves(h, l)
        c = counts.cpu().numpy().astype(np.int64)
        assert int(status.item()) == 0
        assert np.array_equal(np.concatenate([[0], np.cumsum(c)]), off.cpu().numpy())
        take = (torch.arange(rows.shape[1], device=_dev())[None, :] < counts[:, None])
        assert torch.equal(ids[take], cid) and torch.equal(rows[take], crow)
        goff = g["offsets"].astype(np.int64)
        want = np.concatenate([g["ids"][goff[k]:goff[k + 1]] for k in np.flatnonzero(small)]).astype(np.int32)
        assert np.array_equal(ids[take].cpu().numpy(), want)
        counts2, rows2, ids2, status2 = pkg.get_moves_slab(h, l, want_ids=False)     # the launch without an id buffer
        assert ids2 is None and int(status2.item()) == 0 and torch.equal(counts2, counts) and torch.equal(rows2[take], crow)
        off2, crow2, cid2 = pkg.get_moves(h, l, want_ids=False)
        assert cid2 is None and torch.equal(off2, off) and torch.equal(crow2, crow)
    bad_last = torch.zeros((3, 15), dtype=torch.int8); bad_last[1, 0] = 1; bad_last[1, 2] = 1     # "3 5": no combo
    hand = torch.zeros((3, 15), dtype=torch.int8); hand[:, :13] = 1; hand[2, :13] = 4; hand[2, 13:] = 1  # query 2: the full deck
    counts, rows, ids, status = pkg.get_moves_slab(hand.to(_dev()), bad_last.to(_dev()))
    assert counts.tolist()[1] == 0 and counts.tolist()[2] == 0 and counts.tolist()[0] > 13 and int(status.item()) == 6


def test_step_onehot_matches_step_choice(pkg):
    """batched step_manual with [T,15,4] thermometer actions == stepping by list index"""
    T = 1024
    a = pkg.BatchedEnv(T, seed=23); b = pkg.BatchedEnv(T, seed=23)
    a.reset(); b.reset()
    g = torch.Generator().manual_seed(3)
    for _ in range(40):
        offsets, rows, _ = a.legal()
        b.legal()
        A = offsets.diff().cpu()
        choice = (torch.randint(0, 1 << 30, (T,), generator=g) % A.clamp(min=1)).int()
        picked = rows[(offsets[:-1].cpu().long() + choice.long()).to(rows.device)]
        onehot = pkg.rows_to_onehot(picked)                     # [T,15,4] f32, as valid_actions gives
        d1, r1, i1 = a.step(choice, pkg.STEP_CHOICE)
        d2, r2, i2 = b.step_onehot(onehot)
        assert torch.equal(d1, d2) and torch.equal(r1, r2) and not i2.any().item()
        assert torch.equal(a.state, b.state)


def test_serving_payload_inputs(pkg, oracle):
    """face / legal moves computed from the reference's serving payload (server/client.py:6-25,
    server/core.py:26-67) equal those of the live tables the payloads were taken from."""
    import importlib
    import json
    serving = importlib.import_module("doudizhu-rl_amd.serving")
    T = 300
    ref = oracle.OracleEnv(T, seed=77)
    ref.reset()
    for _ in range(31):
        ref.legal(); ref.step(oracle.STEP_RANDOM)
    roff, rrows, _ = ref.legal()
    # the exporter (state -> payloads, server/client.py:6-25), through JSON like the HTTP service
    payloads = json.loads(json.dumps(serving.state_to_payloads(ref.state)))
    t = 7
    role = int(ref.field(10)[t, 0])
    assert payloads[t]["role_id"] == role and len(payloads[t]["cur_cards"]) == int(ref.field(role)[t, 15])
    assert payloads[t]["cur_cards"] == [int(x) for x in np.repeat(np.arange(3, 18), ref.field(role)[t, :15].astype(int))]
    assert [payloads[t]["left"][str(r)] for r in range(3)] == [int(ref.field(r)[t, 15]) for r in range(3)]
    # and back: only the actor's hand travels, everything `face` and the legal moves read is there
    back = serving.payloads_to_state(payloads)
    full = ref.state.reshape(T, 11, 16)
    for tt in range(T):
        rr = int(full[tt, 10, 0])
        assert np.array_equal(back[tt, rr], full[tt, rr]) and np.array_equal(back[tt, 3:10, :15], full[tt, 3:10, :15])
    pred = serving.BatchedPredictorInputs()
    face = pred.face(payloads).cpu().numpy()
    assert np.array_equal(face.view(np.uint32), ref.observe(3).view(np.uint32))
    last, offsets, rows = pred.valid_actions(payloads)
    assert np.array_equal(offsets.cpu().numpy(), roff)
    assert np.array_equal(rows.cpu().numpy(), rrows)
    t = 5
    role = payloads[t]["role_id"]
    prev = payloads[t]["last_taken"][str((role + 2) % 3)]
    assert last[t] == (prev or payloads[t]["last_taken"][str((role + 1) % 3)])


def test_state_export_import_and_determinism(pkg):
    env = pkg.BatchedEnv(2048, seed=5)
    env.reset()
    env.rollout_random(30)
    snap = env.state_export()
    env.rollout_random(30)
    a = env.state_export()
    env2 = pkg.BatchedEnv(2048, seed=5)
    env2.state_import(snap)
    env2.rollout_random(30)
    assert torch.equal(a, env2.state_export())


def test_env_view_matches_reference_api(pkg, oracle):
    """N = 1 drop-in surface of envi.py (shapes, dtypes, return conventions)."""
    env = pkg.EnvCooperationSimplify(seed=1234)
    ref = oracle.OracleEnv(1, seed=1234)
    env.reset(); env.prepare(); ref.reset()
    assert env.get_role_ID() == 2 and env.left.tolist() == [17, 20, 17]        # lord, 1-based
    assert len(env.get_curr_handcards()) == 20
    assert env.get_last_two_cards() == [[], []] and env.get_last_outcards().tolist() == []    # a lead: nothing to beat
    face = env.face
    assert face.dtype == torch.float32 and tuple(face.shape) == (6, 15, 4) and face.is_cuda
    acts = env.valid_actions()
    assert acts.dtype == torch.float32 and acts.shape[1:] == (15, 4) and acts.is_cuda
    _, _, rids = ref.legal()
    lst = env.valid_actions(tensor=False)
    assert len(lst) == len(rids) == acts.shape[0]
    # face + valid_actions come from one library call per ply (ddz_observe_actions); reading a property again in the same
    # ply gives a fresh, equal tensor -- never the one handed out before
    face2, acts2 = env.face, env.valid_actions()
    assert face2.data_ptr() != face.data_ptr() and torch.equal(face2, face)
    assert acts2.data_ptr() != acts.data_ptr() and torch.equal(acts2, acts)
    assert np.array_equal(acts.cpu().numpy().sum(-1).astype(int), np.stack(lst))
    hand_before = env.get_curr_handcards()
    r, done, _ = env.step_manual(acts[-1])
    assert np.array_equal(env.old_cards[1], hand_before) and list(env.old_cards.items())[0][0] == 1   # envi.py:65
    assert (r, done) == (0, False) and env.get_role_ID() == 3                  # down moves next
    assert env.taken.sum() == 20 - env.left[1] and env.history[1].sum() == env.taken.sum()
    # get_last_outcards(): what `down` has to beat = the lord's play as ranks 3..17 (envi.py:103-109; the `last_cards`
    # of rule_based/utils/utils.py:197)
    played = env.arr2cards(env.onehot2arr(acts[-1]))
    assert env.get_last_outcards().tolist() == played.tolist() == env.get_last_two_cards()[0]
    assert np.array_equal(env.cards2arr(env.get_last_outcards()), env.recent_handout[1])
    with pytest.raises(ValueError):
        env.step_manual(torch.ones((15, 4)))                                    # never legal
    done = False
    plies = 0
    while not done:
        r, done, _ = env.step_random()
        plies += 1
    assert r in (-1, 1) and 0 in env.left.tolist() and plies < 170


def _plane_rich_hands(rng, n, cards):
    """Random `cards`-card hands biased towards runs of triples / bombs (SURVEY 8d stress set:
    the compaction worst case, lists of several hundred moves)."""
    hands = np.zeros((n, 15), np.int8)
    for i in range(n):
        h = np.zeros(15, np.int64)
        start = rng.integers(0, 8)
        run = rng.integers(2, 6)
        h[start:start + run] = rng.choice([3, 3, 3, 4], size=run)
        left = cards - int(h.sum())
        while left > 0:
            r = rng.integers(0, 15)
            cap = 1 if r >= 13 else 4
            if h[r] < cap:
                h[r] += 1
                left -= 1
        while h.sum() > cards:
            r = rng.integers(0, 15)
            if h[r] > 0:
                h[r] -= 1
        hands[i] = h
    return hands


@pytest.mark.parametrize("cards", [20, 17, 12])
def test_get_moves_plane_rich_stress(pkg, oracle, golden, cards):
    """Lead and follow lists of plane-rich hands (long lists, many kicker blocks) vs the oracle,
    ids and rows, bit-exact; every category of `last` that such hands can answer."""
    rng = np.random.default_rng(100 + cards)
    table = golden("action_table.npz")
    n = 600
    hands = _plane_rich_hands(rng, n, cards)
    lasts = np.zeros((n, 15), np.int8)
    # a third lead, the rest follow a random action of a random category (small values: beatable)
    cat = table["cat_range"]
    for i in range(n):
        if i % 3 == 0:
            continue
        c = rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14])
        pool = np.nonzero(cat == c)[0]
        lasts[i] = table["rows"][pool[rng.integers(0, max(1, len(pool) // 3))]]
    offsets, rows, ids = pkg.get_moves(torch.from_numpy(hands).to(_dev()), torch.from_numpy(lasts).to(_dev()))
    offsets, rows, ids = offsets.cpu().numpy(), rows.cpu().numpy(), ids.cpu().numpy()
    longest = 0
    for i in range(n):
        want = oracle.legal(hands[i], lasts[i] if lasts[i].any() else None)
        got = ids[offsets[i]:offsets[i + 1]]
        assert np.array_equal(got, want), (i, hands[i], lasts[i])
        assert np.array_equal(rows[offsets[i]:offsets[i + 1], :15], table["rows"][want])
        longest = max(longest, len(want))
    assert longest > (150 if cards >= 17 else 40)  # the stress set does produce long lists


def test_dqn_training_example_runs(pkg):
    """N2 end to end: legal -> observe -> ragged Q -> select -> transitions -> TD step, 256 tables."""
    import importlib.util
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("cfg3train", os.path.join(repo, "examples", "config3_dqn_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--tables", "256", "--iters", "60"])
    assert out["status"] == 0 and out["replay"] > 256 and out["episodes"] > 0
    assert out["last_loss"] is not None and np.isfinite(out["last_loss"])


def _joker_hands(rng, n, cards):
    """hands that hold both jokers and are rich in quads / adjacent triples"""
    hands = _plane_rich_hands(rng, n, cards - 2)
    hands[:, 13:] = 0
    for i in range(n):
        while hands[i].sum() > cards - 2:
            r = rng.choice(np.flatnonzero(hands[i, :13] > 0))
            hands[i, r] -= 1
        while hands[i].sum() < cards - 2:
            r = rng.choice(np.flatnonzero(hands[i, :13] < 4))
            hands[i, r] += 1
    hands[:, 13:] = 1
    return hands


def test_joker_kicker_build_vs_oracle(pkg, oracle):
    """The optional rule set (24 extra rows, default off): lists of the jk library == jk oracle, as lead,
    as follow of an ordinary FOUR_TAKE_ONE / 2-plane and as follow of one of the extra rows; lock-step
    episodes stay bit-identical; the default library never emits an extra id."""
    rng = np.random.default_rng(77)
    n = 400
    hands = _joker_hands(rng, n, 20)
    with oracle.variant(jk=True):
        rows_t, info_t = oracle.action_table()
        lasts = np.zeros((n, 15), np.int8)
        pools = {13: np.flatnonzero(info_t[:, 0] == 13), 10: np.flatnonzero((info_t[:, 0] == 10) & (info_t[:, 2] == 2))}
        for i in range(n):
            if i % 4 == 1:
                lasts[i] = rows_t[rng.choice(pools[13][pools[13] < 13527][:400]), :15]
            elif i % 4 == 2:
                lasts[i] = rows_t[rng.choice(pools[10][pools[10] < 13527][:300]), :15]
            elif i % 4 == 3:
                lasts[i] = rows_t[rng.integers(13527, 13551), :15]   # an extra row was played
        offsets, rows, ids = pkg.get_moves(torch.from_numpy(hands).to(_dev()), torch.from_numpy(lasts).to(_dev()),
                                           native_joker_kickers=True)
        offsets, rows, ids = offsets.cpu().numpy(), rows.cpu().numpy(), ids.cpu().numpy()
        extras = 0
        for i in range(n):
            want = oracle.legal(hands[i], lasts[i] if lasts[i].any() else None)
            got = ids[offsets[i]:offsets[i + 1]]
            assert np.array_equal(got, want), (i, hands[i], lasts[i])
            assert np.array_equal(rows[offsets[i]:offsets[i + 1], :15], rows_t[want, :15])
            assert np.array_equal(rows[offsets[i]:offsets[i + 1], 15].astype(np.uint8), info_t[want, 0])
            extras += int((want >= 13527).sum())
        assert extras > 200
        # lock-step env parity under the extension (state, lists, results every iteration)
        T = 256
        env = pkg.BatchedEnv(T, seed=9, device=_dev(), native_joker_kickers=True)
        ref = oracle.OracleEnv(T, seed=9)
        env.reset(); ref.reset()
        seen = 0
        for it in range(150):
            off, rws, idz = env.legal()
            ref.legal()
            tot = int(off[-1])
            assert np.array_equal(off.cpu().numpy(), ref.offsets)
            assert np.array_equal(idz[:tot].cpu().numpy(), ref.ids[:tot])
            seen += int((ref.ids[:tot] >= 13527).sum())
            done, r, _ = env.step(None, pkg.STEP_RANDOM, auto_reset=True)
            rdone, rr = ref.step(oracle.STEP_RANDOM, auto_reset=True)[:2]
            assert np.array_equal(done.cpu().numpy(), rdone) and np.array_equal(r.cpu().numpy(), rr)
        assert np.array_equal(env.state_export().cpu().numpy(), ref.state)
        env2 = pkg.BatchedEnv(T, seed=9, device=_dev(), native_joker_kickers=True)
        env2.reset()
        env2.rollout_random(150)
        assert torch.equal(env2.state_export(), env.state_export()) and env2.status() == 0
    # default library: same hands, no id of the extension
    _, _, ids0 = pkg.get_moves(torch.from_numpy(hands).to(_dev()), torch.zeros((n, 15), dtype=torch.int8, device=_dev()))
    assert int(ids0.max()) < 13527


@pytest.mark.parametrize("T,iters,seed,base", [(700, 220, 3, 0), (4096, 60, 11, 2**40)])
def test_slab_api_lockstep_vs_oracle(pkg, oracle, T, iters, seed, base):
    """legal_slab / step_slab (one launch per iteration) vs the oracle's legal / step with the same
    choices: lists (sizes, ids, rows), done / r / illegal and the full state every iteration; CHOICE with
    valid, out-of-range and negative indices, ROWS every few iterations, no auto-reset on some of them."""
    rng = np.random.default_rng(seed)
    env = pkg.BatchedEnv(T, seed=seed, device=_dev(), table_id_base=base)
    ref = oracle.OracleEnv(T, seed=seed, gid_base=base)
    env.reset(); ref.reset()
    counts, rows, ids = env.legal_slab()
    for it in range(iters):
        roff, rrows, rids = ref.legal()
        n = np.diff(roff)
        c = counts.cpu().numpy()
        assert np.array_equal(c, n)
        idn = ids.cpu().numpy(); rwn = rows.cpu().numpy()
        take = np.arange(env.slab_stride)[None, :] < n[:, None]
        assert np.array_equal(idn[take], rids)
        assert np.array_equal(rwn[take], rrows)
        choice = (rng.random(T) * np.maximum(n, 1)).astype(np.int32)
        bad = rng.random(T) < 0.03
        choice[bad] = np.where(rng.random(bad.sum()) < 0.5, -1, n[bad] + rng.integers(0, 3, bad.sum()))
        auto = it % 5 != 4
        if it % 7 == 3:   # ROWS: the chosen rows themselves (bad ones: a row that is not in the list)
            ok = (choice >= 0) & (choice < n)
            sel_rows = np.zeros((T, 16), np.int8)
            sel_rows[ok] = rrows[roff[:-1][ok] + choice[ok]]
            sel_rows[~ok, 0] = 7
            done, r, ill = env.step_slab(torch.from_numpy(sel_rows).to(_dev()), pkg.STEP_ROWS, auto_reset=auto)
            rdone, rr, rill, _ = ref.step(oracle.STEP_ROWS, sel_rows, auto_reset=auto)
        else:
            done, r, ill = env.step_slab(torch.from_numpy(choice).to(_dev()), pkg.STEP_CHOICE, auto_reset=auto)
            rdone, rr, rill, _ = ref.step(oracle.STEP_CHOICE, choice, auto_reset=auto)
        assert np.array_equal(done.cpu().numpy(), rdone) and np.array_equal(r.cpu().numpy(), rr)
        assert np.array_equal(ill.cpu().numpy(), rill)
        assert np.array_equal(env.state_export().cpu().numpy(), ref.state)
        if it % 20 == 19:  # finished tables stay frozen without auto-reset until reset(mask)
            m = (env.field(10)[:, 1] != 0)
            env.reset(mask=m); ref.reset(m.cpu().numpy().astype(np.uint8))
            counts, rows, ids = env.legal_slab()
    assert env.status() == 0
    st = env.stats()
    assert st["plies"] > 0 and st["episodes"] > 0


@pytest.mark.parametrize("T,want_ids", [(1500, True), (4096, False), (37, True)])
def test_slab_block_written_lists_equal_single_wave_lists(pkg, oracle, T, want_ids):
    """One table per wave (T <= 4096): the lists of plane-rich leads -- the lord's 20-card lead of a fresh game above all
    -- are written by all sixteen waves of the block (slab_list_team: the scan rounds dealt out, counted, scanned, written
    at their bases), every other list by the table's own wave, deals by the table's wave.  Same games, byte-identical
    slabs as the form in which one wave writes each list (ddz_debug_set_geometry slab_coop = 2) and as the
    many-tables-per-wave form; the heaviest lists against the oracle."""
    a = pkg.BatchedEnv(T, seed=77, device=_dev(), want_ids=want_ids)                              # block-written heavy lists
    b = pkg.BatchedEnv(T, seed=77, device=_dev(), want_ids=want_ids, _debug_slab_coop=2)          # one wave per list
    c = pkg.BatchedEnv(T, seed=77, device=_dev(), want_ids=want_ids, _debug_tables_per_wave=3)    # work-list form
    ref = oracle.OracleEnv(T, seed=77)
    for e in (a, b, c):
        e.reset(); e.legal_slab()
    ref.reset()
    S = a.slab_stride
    heavy_seen = 0
    for it in range(260):
        for e in (a, b, c):
            e.step_slab(None, pkg.STEP_RANDOM, auto_reset=True)
        ref.legal(); ref.step(oracle.STEP_RANDOM, None, auto_reset=True)
        ca = a.counts.cpu().numpy()
        assert np.array_equal(ca, b.counts.cpu().numpy()) and np.array_equal(ca, c.counts.cpu().numpy()), it
        take = (torch.arange(S, device=_dev())[None, :] < a.counts[:, None]).reshape(-1)
        n = T * S   # (the buffers are sized for the largest stride: rows [cap][16], ids [cap])
        assert torch.equal(a.rows[:n][take], b.rows[:n][take]) and torch.equal(a.rows[:n][take], c.rows[:n][take]), it
        if want_ids:
            assert torch.equal(a.ids[:n][take], b.ids[:n][take]) and torch.equal(a.ids[:n][take], c.ids[:n][take]), it
        assert torch.equal(a.state, b.state) and torch.equal(a.state, c.state), it
        heavy_seen += int((ca > 60).sum())
        if it % 13 == 0 or it > 250:
            roff, rrows, rids = ref.legal()
            assert np.array_equal(a.state.cpu().numpy(), ref.state), it
            assert np.array_equal(ca, np.diff(roff)), it
            assert np.array_equal(a.rows[:n].cpu().numpy()[take.cpu().numpy()], rrows), it
            if want_ids:
                assert np.array_equal(a.ids[:n].cpu().numpy()[take.cpu().numpy()], rids), it
    assert heavy_seen > 0 and a.status() == 0 and b.status() == 0 and c.status() == 0
    assert a.stats() == b.stats() == c.stats()


def test_slab_api_random_equals_rollout(pkg):
    """step_slab(STEP_RANDOM) plays the same games as rollout_random / step_random (same engine RNG)."""
    a = pkg.BatchedEnv(1500, seed=21, device=_dev())
    b = pkg.BatchedEnv(1500, seed=21, device=_dev())
    a.reset(); b.reset()
    for _ in range(90):
        a.step_slab(None, pkg.STEP_RANDOM, auto_reset=True)
    b.rollout_random(90)
    assert torch.equal(a.state_export(), b.state_export())
    sa, sb = a.stats(), b.stats()
    assert sa["plies"] == sb["plies"] and sa["episodes"] == sb["episodes"] and sa["lord_wins"] == sb["lord_wins"]
    assert sa["legal_rows"] >= sb["legal_rows"]   # + the lists of the first legal_slab()


@pytest.mark.parametrize("jk", [False, True])
def test_legal_mask_vs_oracle(pkg, oracle, jk):
    """ddz_legal_mask = the reference's get_mask for every table: bit id set <=> id in the oracle's legal list
    (lead, follow, frozen tables), bit-packed and unpacked forms, default and joker-kicker rule sets."""
    T = 900
    with oracle.variant(jk=jk):
        env = pkg.BatchedEnv(T, seed=31, device=_dev(), native_joker_kickers=jk)
        ref = oracle.OracleEnv(T, seed=31)
        env.reset(); ref.reset()
        na = oracle.num_actions()
        for it in range(60):
            if it % 6 == 0:
                roff, _, rids = ref.legal()
                want = np.zeros((T, na), bool)
                want[np.repeat(np.arange(T), np.diff(roff)), rids] = True
                got = env.legal_mask(unpack=True).cpu().numpy()
                assert got.shape == (T, na) and np.array_equal(got, want)
                packed = env.legal_mask().cpu().numpy().view(np.uint32)
                assert packed.shape == (T, 424)
                assert np.array_equal(np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, :na].astype(bool), want)
                assert not np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, na:].any()
            auto = it < 40   # later: finished tables stay frozen -> all-zero mask rows
            env.step(None, pkg.STEP_RANDOM, auto_reset=auto)
            ref.legal(); ref.step(oracle.STEP_RANDOM, auto_reset=auto)
        frozen = env.field(10)[:, 1].cpu().numpy() != 0
        assert frozen.any() and not env.legal_mask(unpack=True).cpu().numpy()[frozen].any()


@pytest.mark.parametrize("eps", [0.0, 0.3])
def test_select_slab_equals_select(pkg, eps):
    """The slab form of ddz_select picks exactly what the CSR form picks for the same per-move values
    (same arg-max rule, same exploration RNG), and step_slab(choice) == step(choice)."""
    T = 3000
    a = pkg.BatchedEnv(T, seed=5, device=_dev())
    b = pkg.BatchedEnv(T, seed=5, device=_dev())
    a.reset(); b.reset()
    g = torch.Generator(device="cpu").manual_seed(1)
    for it in range(40):
        off, rows, _ = a.legal()
        counts, srows, _ = b.legal_slab()
        n = off.diff().long()
        assert torch.equal(n.to(torch.int32), counts)
        total = int(off[-1])
        q = torch.rand(total, generator=g).to(_dev())
        q[torch.rand(total, generator=g).to(_dev()) < 0.2] = 0.5        # ties: first maximum wins
        seg = torch.repeat_interleave(torch.arange(T, device=_dev()), n, output_size=total)
        pos = torch.arange(total, device=_dev()) - off[:-1].long()[seg]
        qs = torch.full((T, b.slab_stride), 9.0, device=_dev())         # garbage beyond counts must be ignored
        qs[seg, pos] = q
        ca, cb = a.select(q, eps), b.select_slab(qs, eps)
        assert torch.equal(ca, cb)
        da = a.step(ca, pkg.STEP_CHOICE, auto_reset=True)
        db = b.step_slab(cb, pkg.STEP_CHOICE, auto_reset=True)
        assert all(torch.equal(x, y) for x, y in zip(da, db))
    assert torch.equal(a.state_export(), b.state_export())


def test_get_moves_random_sweep(pkg, oracle, golden):
    """4000 random (hand, last) pairs: hands of 1..20 random cards, `last` a uniformly random action of the
    whole action space (every category, every length, including ones the hand cannot answer) or a lead."""
    rng = np.random.default_rng(2024)
    table = golden("action_table.npz")
    deck = np.repeat(np.arange(15), [4] * 13 + [1, 1])
    n = 4000
    hands = np.zeros((n, 15), np.int8)
    lasts = np.zeros((n, 15), np.int8)
    for i in range(n):
        k = int(rng.integers(1, 21))
        hands[i] = np.bincount(rng.choice(deck, k, replace=False), minlength=15)
        if i % 5:
            lasts[i] = table["rows"][rng.integers(1, NA)]
    offsets, rows, ids = pkg.get_moves(torch.from_numpy(hands).to(_dev()), torch.from_numpy(lasts).to(_dev()))
    offsets, ids = offsets.cpu().numpy(), ids.cpu().numpy()
    for i in range(n):
        want = oracle.legal(hands[i], lasts[i] if lasts[i].any() else None)
        assert np.array_equal(ids[offsets[i]:offsets[i + 1]], want), (i, hands[i], lasts[i])
    assert np.array_equal(rows.cpu().numpy()[:, :15], table["rows"][ids])


def test_action_table_and_compact_trajectory(pkg, golden):
    """ddz_action_table == the reference's action space (G1); ddz_pack_trajectory: every field of the 32-byte
    record is recoverable from the 8-byte one (the action through its id and the table)."""
    import importlib
    ddist = importlib.import_module("doudizhu-rl_amd.dist")
    table = golden("action_table.npz")
    rows = pkg.action_table(_dev())
    assert rows.shape == (NA, 16)
    assert np.array_equal(rows[:, :15].cpu().numpy(), table["rows"])
    assert np.array_equal(rows[:, 15].cpu().numpy().astype(np.uint8), table["cat_range"])
    assert pkg.action_table(_dev(), native_joker_kickers=True).shape == (NA + 24, 16)
    T, K = 1200, 120
    env = pkg.BatchedEnv(T, seed=13, device=_dev())
    env.reset()
    traj = torch.zeros((K, T, 32), dtype=torch.uint8, device=_dev())
    for k in range(K):   # some iterations without auto-reset: frozen records appear
        env.step(None, pkg.STEP_RANDOM, auto_reset=(k % 40 < 30), traj=traj[k])
        if k % 40 == 39:
            env.reset(mask=env.field(10)[:, 1] != 0)
    packed = pkg.pack_trajectory(traj)
    assert packed.shape == (K, T, 8) and packed.dtype == torch.uint8
    full = ddist.unpack_trajectory(traj)
    comp = ddist.unpack_trajectory(packed, action_rows=rows)
    for key in ("n_legal", "role", "done", "reward", "flags", "choice", "ply"):
        assert torch.equal(full[key], comp[key]), key
    assert torch.equal(full["episode"] & 0x3FFF, comp["episode"])
    assert torch.equal(comp["row"][..., :15], full["row"][..., :15])
    played = (full["flags"] == 0)
    # a flagged record (frozen table / illegal selection) holds no action: id 0x3FFF, never 0 = the pass (include/ddz_env.h)
    assert torch.equal(comp["id"] == 0x3FFF, ~played) and bool(played.any()) and bool((full["flags"] & 2).any())
    assert int((comp["id"][played] == 0).sum()) > 0   # real passes keep id 0
    assert torch.equal(comp["row"][..., 15][played], full["row"][..., 15][played])
    # single-process gather (world 1): compact=True returns the packed form
    g = ddist.gather_trajectories(traj, compact=True)
    assert torch.equal(g, packed)


def test_misaligned_buffers_are_argument_errors(pkg):
    """Rows / records / planes move as 16-byte words: a misaligned caller pointer is DDZ_EINVAL, not a fault."""
    raw = torch.zeros(64 * 16 + 16, dtype=torch.int8, device=_dev())
    bad = raw[1:1 + 64 * 16].view(64, 16)
    assert bad.data_ptr() % 16 != 0
    with pytest.raises(pkg.DdzError):
        pkg.rows_to_onehot(bad)
    env = pkg.BatchedEnv(64, seed=1, device=_dev())
    env.reset()
    rawf = torch.zeros(64 * 6 * 60 + 4, dtype=torch.float32, device=_dev())
    with pytest.raises(pkg.DdzError):
        env.observe(3, out=rawf[1:1 + 64 * 6 * 60].view(64, 6, 15, 4))
    assert env.status() == 0
    env.observe(3)  # the handle is still fine


def test_bench_contract():
    """bench.py prints ONE JSON line with the driver's keys; the N = 1 workload is the largest single-GPU configuration
    (65,536 tables, the same per-GPU workload as N > 1); the headline roofline (HIP-event launch duration; replayed
    inputs named with their source files) and one roofline block per leg; the CPU baseline; an empty `errors` list."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--full", "--steps", "300", "--warmup", "30",
                        "--cpu-budget", "1.5"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "errors"):
        assert k in j, k
    assert j["errors"] == []
    assert j["n_gpus"] == 1 and j["steps"] == 300 and j["warmup"] == 30 and j["higher_is_better"] is True
    assert j["unit"] == "env steps/s" and j["dtype"] == "u8" and j["scaling"] == "weak" and j["vs_baseline"] is None
    assert j["config"]["tables_per_gpu"] == 65536 and "65536 tables" in j["config"]["workload"]
    assert j["value"] > 1e8 and abs(j["ms_per_step"] * 1e-3 * j["value"] - 65536) < 16
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1 and abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-9
    assert r["kernel"] == "k_rollout" and r["env_steps_per_launch"] == 65536 * r["iterations_per_launch"]
    assert r["traffic"] is None or "profiles/pmc_traffic.json" in r["traffic_source"]          # replayed inputs say so
    assert "workload" in j["config"] and "model" not in j["config"]
    # the headline times exactly the 300 steps asked for; the roofline's own timing is self-sufficient: launches of
    # >= 1000 iterations repeated until >= 50 ms are timed
    assert j["timed_steps"] == 300 and abs(j["timed_seconds"] / 300 * 1e3 - j["ms_per_step"]) < 1e-9
    assert r["iterations_per_launch"] == 1200   # four times the 300 steps: a launch carries >= 1000 iterations
    assert r["launches_timed"] >= 2 and r["launch_us"] * r["launches_timed"] >= 45e3
    # the CSR layout beside the slab layout, at the same table count
    assert j["config"]["csr_env_steps_per_s"] > 1e8 and j["config"]["csr_launch_per_iteration_env_steps_per_s"] > 1e7
    assert 0 < j["config"]["csr_staging_GiB"] <= 17   # the staged CSR rollout's slabs (engine.CSR_STAGING_BYTES)
    assert j["config"]["per_rank_env_steps_per_s"] == [j["value"]]
    iss = r["issue"]
    assert iss is None or (iss["bound"] == "valu-issue" and 0 < iss["frac"] < 1 and "profiles/" in " ".join(iss["sources"].values())
                           and iss["live"] == ["launch_us", "achieved", "frac"])
    legs = j["configs"]
    for k in ("tables_4096_random_rollout", "tables_65536_traj_write_pack", "tables_65536_policy_loop_slab",
              "tables_65536_policy_loop_fused", "tables_65536_dqn_inference", "tables_65536_step_slab_only",
              "tables_65536_step_slab_csr_lists", "tables_65536_rule_opponent"):
        assert legs[k]["env_steps_per_s"] > 1e6, (k, legs[k])
        rf = legs[k]["roofline"]                                  # every leg carries the roof of its dominant kernel
        assert rf["bound"] in ("hbm", "mfma") and rf["peak"] in (8000.0, 157.3) and 0 < rf["frac"] < 1 and rf["launch_us"] > 0, k
    s4 = legs["tables_4096_step_slab_only"]                       # the policy-driven launch at configs[1]'s size (one table per wave)
    assert s4["env_steps_per_s"] > 1e8 and 0 < s4["us_per_launch_events"] < 14 and s4["roofline"]["kernel"] == "k_slab<0,true,true>"
    small = legs["tables_4096_random_rollout"]                    # configs[1] as BASELINE.json writes it
    assert small["roofline"]["env_steps_per_launch"] == 4096 * 1000 and small["csr_env_steps_per_s"] > 1e8
    for k in ("tables_65536_step_slab_only", "tables_65536_rule_opponent", "tables_65536_policy_loop_fused"):
        iss = legs[k]["roofline"]["issue"]
        assert iss is None or (iss["bound"] == "valu-issue" and iss["frac"] > 0)
    dq = legs["tables_65536_dqn_inference"]
    assert dq["roofline"]["bound"] == "mfma" and dq["roofline"]["dtype"] == "f32" and dq["env_steps_per_s"] > 5e6
    st = dq["roofline"]["stages"]
    assert {"need", "shared_rows", "features_shared", "features", "shared_need", "fc1_shared", "gather_h0", "fc1_rows", "row_stage",
            "env_step"} <= set(st)
    assert st["fc1_shared"]["bound"] == "mfma" and st["fc1_rows"]["kernel"] == "k_fc1<true>" and st["features"]["bound"] == "hbm"
    assert {"needed_dense_gemm_by_k_fc1_env_steps_per_s", "needed_dense_gemm_by_hipblaslt_env_steps_per_s"} <= set(dq["variants"])
    assert dq["roofline"]["dense_form_flop"] > dq["roofline"]["executed_flop"] > 0
    # (the stages are timed one after the other; in the loop the D chain runs on a side stream beside the H0 chain)
    assert 0.6 * dq["us_per_iteration"] < sum(dq["stages_us"].values()) < 1.5 * dq["us_per_iteration"]
    ret = legs["tables_65536_rule_opponent"]["mean_episode_return"]
    assert ret["up"] == ret["down"] == -ret["lord"] / 2 and ret["lord"] < -50  # rule farmers beat a random lord
    c = j["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 1e4 and "sample" in c


def test_bench_plain_run_times_k_steps_and_dumps_them(pkg, tmp_path):
    """A plain bench.py run is the headline alone: exactly --steps timed steps, none of --full's figures.  Its
    --dump-outputs files are the same in two runs and equal an independent rollout of warmup + steps iterations."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    T, K, W = 4096, 50, 7
    runs = []
    for name in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--tables", str(T), "--steps", str(K),
                            "--warmup", str(W), "--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        assert len(lines) == 1 and len(lines[0]) < 4000
        runs.append(json.loads(lines[0]))
    j = runs[0]
    assert j["steps"] == K and j["timed_steps"] == K and j["warmup"] == W and j["value"] > 0 and j["errors"] == []
    assert abs(j["ms_per_step"] * 1e-3 * j["value"] - T) < 1e-6 * T
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(j)
    assert not {"roofline", "configs", "cpu_baseline"} & set(j) and "exchange" not in j["config"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "state.npy" in names
    out = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        assert out[n[:-4]].dtype in (np.float32, np.float64), n
        assert np.array_equal(out[n[:-4]], np.load(tmp_path / "b" / n)), n
    env = pkg.BatchedEnv(T, seed=0, device=_dev(), want_ids=False)
    env.reset()
    env.rollout_random(W)
    env.rollout_random(K)
    assert np.array_equal(out["state"], env.state.view(T, -1, 16).float().cpu().numpy())
    counts = env.counts.cpu().numpy()
    assert np.array_equal(out["legal_counts"], counts.astype(np.float32))
    tabs = out["legal_rows_tables"].astype(np.int64)
    rows = env.slab_rows().cpu().numpy()
    assert np.array_equal(out["legal_rows"], np.concatenate([rows[t, :counts[t]] for t in tabs]).astype(np.float32))
    assert out["stats"][0] == T * (W + K) and out["stats"][1] == env.stats()["episodes"]


def test_bench_two_ranks_rehearsal_gathers_the_union(pkg):
    """The N > 1 control flow of bench.py (shard ids, packed trajectory gather to rank 0, two pipelined half-batches)
    executed by two processes on this one GPU (gloo, host-staged: a rehearsal, not a measurement): the records rank 0
    gathered equal a single-process rollout of the union of the two shards, record for record."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    T, K, W, KX = 512, 40, 10, 30
    env_ = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    # exactly what the driver types: no launcher here -- bench.py starts its two ranks itself (spawn_ranks)
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--full", "--gpus", "2", "--rehearse", "--tables", str(T),
                        "--steps", str(K), "--warmup", str(W), "--exchange-steps", str(KX)],
                       capture_output=True, text=True, timeout=600, env=env_)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    ex = j["config"]["exchange"]
    assert j["n_gpus"] == 2 and j["config"]["total_tables"] == 2 * T and "error" not in ex
    assert ex["steps"] == KX and ex["bytes_to_rank0"] == KX * T * 8 and j["env_steps_per_s_with_gather"] > 0
    env = pkg.BatchedEnv(2 * T, seed=0, device=_dev(), want_ids=False)
    env.reset()
    env.rollout_random(ex["iterations_before"])
    half = KX // 2
    ta = torch.zeros((half, 2 * T, 32), dtype=torch.uint8, device=_dev())
    tb = torch.zeros((KX - half, 2 * T, 32), dtype=torch.uint8, device=_dev())
    env.rollout_random(half, traj=ta)
    env.rollout_random(KX - half, traj=tb)
    x = torch.cat([pkg.pack_trajectory(ta), pkg.pack_trajectory(tb)]).contiguous().view(torch.int64).view(-1)
    digest = int((x * 31 + (x >> 13) + torch.arange(x.numel(), device=_dev()) * x).sum().item())
    assert digest == ex["digest"]


def test_rccl_collectives_of_the_exchange_on_one_rank(pkg):
    """The end-of-batch exchange through the REAL backend: a one-rank `nccl` (= RCCL) process group on this GPU, created
    the way bench.py creates it (init_process_group("nccl", device_id=...)), runs the exact collectives of
    dist.gather_trajectories -- gather of uint8 records to the learner rank (asynchronous, two batches in flight),
    all_gather_into_tensor, the size exchange, barrier, all_reduce of the timing scalars -- and returns the records
    unchanged.  (Several ranks need several GPUs: the driver's SCALE run; world-2 semantics are covered on gloo.)"""
    import os
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    code = r"""
import datetime, importlib, os, sys
import torch, torch.distributed as dist
sys.path.insert(0, %r)
pkg = importlib.import_module("doudizhu-rl_amd"); ddist = importlib.import_module("doudizhu-rl_amd.dist")
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=datetime.timedelta(minutes=2))
T, K = 3000, 12
env = pkg.BatchedEnv(T, seed=3, device=dev, want_ids=False); env.reset()
traj = torch.zeros((K, T, 32), dtype=torch.uint8, device=dev)
env.rollout_random(K, traj=traj)
packed = pkg.pack_trajectory(traj)
dist.barrier(); torch.cuda.synchronize(dev)
h1 = ddist.gather_trajectories(packed[: K // 2].contiguous(), dst=0, async_op=True, shard_sizes=[T], _force_collective=True)
h2 = ddist.gather_trajectories(packed[K // 2:].contiguous(), dst=0, async_op=True, shard_sizes=[T], _force_collective=True)
got = torch.cat([h1.result(), h2.result()])
assert torch.equal(got, packed)
full = ddist.gather_trajectories(traj, _force_collective=True)              # all_gather + size exchange, 32-byte records
assert torch.equal(full, traj)
comp = ddist.gather_trajectories(traj, dst=0, compact=True, _force_collective=True)
assert torch.equal(comp, packed)
t = torch.tensor([1.5], dtype=torch.float64, device=dev); dist.all_reduce(t, op=dist.ReduceOp.MAX); assert float(t) == 1.5
rec = ddist.unpack_trajectory(got[-1])
assert int(rec["role"].max()) <= 2 and int(rec["id"][rec["flags"] == 0].max()) < 13527
dist.barrier(); dist.destroy_process_group()
print("RCCL_OK", dist.Backend.NCCL)
""" % repo
    env_ = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env_.pop(k, None)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env_)
    assert p.returncode == 0 and "RCCL_OK" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])


def test_slab_to_csr_equals_legal(pkg):
    """ddz_slab_to_csr: the slab lists packed to CSR are byte-identical to ddz_legal's offsets / rows / ids on the same
    states (ragged sizes, mid-game and fresh deals, a table count that is not a multiple of the block), a choice index
    means the same move in both layouts, and an undersized buffer raises status bit 1 without writing past it."""
    import torch
    for T in (1, 257, 5000):
        env = pkg.BatchedEnv(T, seed=31 + T, device=torch.device("cuda:0"))
        env.reset()
        env.rollout_random(7)
        for rpt in (512,):
            env.legal_slab()
            off, rows, ids = env.slab_to_csr(rows_per_table=rpt)
            off, tot = off.clone(), int(off[-1].item())
            rows, ids = rows[:tot].clone(), ids[:tot].clone()
            off2, rows2, ids2 = env.legal()
            assert torch.equal(off, off2) and int(off2[-1].item()) == tot
            assert torch.equal(rows, rows2[:tot]) and torch.equal(ids, ids2[:tot])
        assert env.status() == 0
    env = pkg.BatchedEnv(900, seed=6, device=torch.device("cuda:0"), want_ids=False)   # no id buffers at all
    env.reset()
    env.rollout_random(11)
    env.legal_slab()
    off, rows, ids = env.slab_to_csr(rows_per_table=512)
    assert ids is None
    off, tot = off.clone(), int(off[-1].item())
    rows = rows[:tot].clone()
    off2, rows2, _ = env.legal()
    assert torch.equal(off, off2) and torch.equal(rows, rows2[:tot]) and env.status() == 0
    env = pkg.BatchedEnv(300, seed=5, device=torch.device("cuda:0"))
    env.reset()
    env.legal_slab()
    total = int(env.counts.sum().item())
    off, rows, ids = env.slab_to_csr(rows_per_table=8)          # a fresh lead has ~73 legal moves: 2400 rows do not fit
    # truncated: status bit 1, and the offsets are clamped to the capacity (every segment stays inside the buffer)
    assert total > 2400 and int(off[-1].item()) == 2400 and int(off.max().item()) == 2400 and env.status() & 2
    off = off.clone()
    off2, rows2, ids2 = env.legal()
    assert torch.equal(rows[:2400], rows2[:2400]) and torch.equal(ids[:2400], ids2[:2400])
    assert torch.equal(off, off2.clamp(max=2400))


def test_slab_to_csr_select_step_slab_runs_no_second_enumeration(pkg, oracle):
    """The advertised CSR policy loop: step_slab -> slab_to_csr -> q over the CSR rows -> select(q) -> step_slab(CHOICE).
    select() must take the offsets slab_to_csr just wrote (no ddz_legal, which would also overwrite the slab buffer and
    force step_slab to enumerate again): legal() / legal_slab() are called exactly once (the initial lists), and states,
    lists and choices equal the oracle's every iteration."""
    T = 700
    env = pkg.BatchedEnv(T, seed=23, device=_dev())
    ref = oracle.OracleEnv(T, seed=23)
    env.reset(); ref.reset()
    calls = {"legal": 0, "legal_slab": 0}
    real_legal, real_slab = env.legal, env.legal_slab

    def counting(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    env.legal, env.legal_slab = counting("legal", real_legal), counting("legal_slab", real_slab)
    env.legal_slab()
    g = torch.Generator().manual_seed(4)
    for it in range(40):
        off, rows, ids = env.slab_to_csr(rows_per_table=512)
        roff, rrows, rids = ref.legal()
        n = int(roff[-1])
        assert np.array_equal(off.cpu().numpy(), roff) and np.array_equal(ids[:n].cpu().numpy(), rids)
        q = torch.randint(-3, 4, (T * 512,), generator=g).float()
        choice = env.select(q.to(_dev()))
        want = np.array([int(np.argmax(q[roff[t]:roff[t + 1]].numpy())) if roff[t + 1] > roff[t] else -1 for t in range(T)], np.int32)
        assert np.array_equal(choice.cpu().numpy(), want)
        env.step_slab(choice, pkg.STEP_CHOICE, auto_reset=True)
        ref.step(oracle.STEP_CHOICE, want, auto_reset=True)
        assert np.array_equal(env.state.cpu().numpy(), ref.state), it
    assert calls == {"legal": 0, "legal_slab": 1} and env.status() == 0


def test_slab_api_all_modes_large_batch_vs_oracle(pkg, oracle):
    """k_slab at a large batch with the default geometry (70,001 tables: 18 tables per wave = a full chunk of 16 + 2, a
    ragged last wave) x 10 iterations in every mode against the oracle on ALL tables: lists, outputs, full state."""
    T, seed = 70001, 908
    rng = np.random.default_rng(seed)
    env = pkg.BatchedEnv(T, seed=seed, device=_dev())
    ref = oracle.OracleEnv(T, seed=seed)
    env.reset(); ref.reset()
    env.rollout_random(23); ref.rollout_random(23)      # desynchronised mid-game states, some games already finished
    counts, rows, ids = env.legal_slab()
    for it in range(10):
        roff, rrows, rids = ref.legal()
        n = np.diff(roff)
        assert np.array_equal(counts.cpu().numpy(), n)
        if it % 5 == 0:
            take = np.arange(env.slab_stride)[None, :] < n[:, None]
            assert np.array_equal(ids.cpu().numpy()[take], rids) and np.array_equal(rows.cpu().numpy()[take], rrows)
        mode = (pkg.STEP_CHOICE, pkg.STEP_IDS, pkg.STEP_RANDOM, pkg.STEP_ROWS)[it % 4]
        choice = (rng.random(T) * np.maximum(n, 1)).astype(np.int32)
        bad = rng.random(T) < 0.02
        choice[bad] = -1
        pick = roff[:-1] + np.clip(choice, 0, np.maximum(n - 1, 0))
        if mode == pkg.STEP_CHOICE:
            sel, rsel = torch.from_numpy(choice), choice
        elif mode == pkg.STEP_IDS:
            v = np.where(bad, -1, rids[np.minimum(pick, len(rids) - 1)]).astype(np.int32)   # -1: engine RNG
            sel, rsel = torch.from_numpy(v), v
        elif mode == pkg.STEP_ROWS:
            v = rrows[np.minimum(pick, len(rrows) - 1)].copy()
            v[bad] = 9                                  # no such move: illegal
            sel, rsel = torch.from_numpy(v), v
        else:
            sel, rsel = None, None
        done, rew, ill = env.step_slab(sel.to(_dev()) if sel is not None else None, mode, auto_reset=it % 3 != 2)
        rdone, rrew, rill, _ = ref.step({pkg.STEP_CHOICE: oracle.STEP_CHOICE, pkg.STEP_IDS: oracle.STEP_IDS,
                                         pkg.STEP_RANDOM: oracle.STEP_RANDOM, pkg.STEP_ROWS: oracle.STEP_ROWS}[mode],
                                        rsel, auto_reset=it % 3 != 2)
        assert np.array_equal(done.cpu().numpy(), rdone) and np.array_equal(rew.cpu().numpy(), rrew)
        assert np.array_equal(ill.cpu().numpy(), rill)
        assert np.array_equal(env.state.cpu().numpy(), ref.state), (it, mode)
        if it % 3 == 2:
            env.reset(mask=done); ref.reset(mask=rdone)
            counts, rows, ids = env.legal_slab()
    assert env.status() == 0


@pytest.mark.parametrize("tpw", [1, 5, 16, 23, 40, -16])
def test_slab_api_chunks_and_modes_vs_oracle(pkg, oracle, tpw):
    """k_slab handles a wave's tables in lane-parallel chunks of 16: every chunking (one table per wave, a partial chunk,
    exactly one, 16 + 7, 16 + 16 + 8; the last wave ragged) x every mode (CHOICE, ROWS, IDS with engine draws, RANDOM)
    against the oracle: lists, done / r / illegal, trajectory records and the full state after every iteration."""
    work_list = tpw > 0       # (-16: 16 tables per wave WITHOUT the block work list of deals + lists: every wave its own)
    tpw = abs(tpw)
    T, seed = 1003, 40 + tpw
    rng = np.random.default_rng(seed)
    env = pkg.BatchedEnv(T, seed=seed, device=_dev(), _debug_tables_per_wave=tpw, _debug_slab_work_list=work_list)  # ddz_debug_set_geometry
    ref = oracle.OracleEnv(T, seed=seed)
    env.reset(); ref.reset()
    counts, rows, ids = env.legal_slab()
    traj = torch.zeros((T, 32), dtype=torch.uint8, device=_dev())
    for it in range(48):
        roff, rrows, rids = ref.legal()
        n = np.diff(roff)
        assert np.array_equal(counts.cpu().numpy(), n)
        take = np.arange(env.slab_stride)[None, :] < n[:, None]
        assert np.array_equal(ids.cpu().numpy()[take], rids) and np.array_equal(rows.cpu().numpy()[take], rrows)
        choice = (rng.random(T) * np.maximum(n, 1)).astype(np.int32)
        bad = rng.random(T) < 0.04
        choice[bad] = np.where(rng.random(bad.sum()) < 0.5, -1, n[bad] + rng.integers(0, 3, bad.sum()))
        ok = (choice >= 0) & (choice < n)
        auto = it % 6 != 5
        mode = it % 4
        if mode == 0:
            sel, gm, om = choice, pkg.STEP_CHOICE, oracle.STEP_CHOICE
        elif mode == 1:
            sel = np.zeros((T, 16), np.int8)
            sel[ok] = rrows[roff[:-1][ok] + choice[ok]]
            sel[ok, 15] = 0                                   # the caller's rows carry no category byte
            sel[~ok, 0] = 7
            gm, om = pkg.STEP_ROWS, oracle.STEP_ROWS
        elif mode == 2:
            sel = np.full(T, 13600, np.int32)                 # no such action
            sel[ok] = rids[roff[:-1][ok] + choice[ok]]
            draw = rng.random(T) < 0.3
            sel[draw] = -1                                    # engine RNG for these tables
            gm, om = pkg.STEP_IDS, oracle.STEP_IDS
        else:
            sel, gm, om = None, pkg.STEP_RANDOM, oracle.STEP_RANDOM
        done, r, ill = env.step_slab(None if sel is None else torch.from_numpy(sel).to(_dev()), gm, auto_reset=auto, traj=traj)
        rdone, rr, rill, rtraj = ref.step(om, sel, auto_reset=auto, want_traj=True)
        assert np.array_equal(done.cpu().numpy(), rdone) and np.array_equal(r.cpu().numpy(), rr), (tpw, it)
        assert np.array_equal(ill.cpu().numpy(), rill), (tpw, it)
        assert np.array_equal(traj.cpu().numpy(), rtraj), (tpw, it)
        assert np.array_equal(env.state_export().cpu().numpy(), ref.state), (tpw, it)
        if it % 12 == 11:
            m = (env.field(10)[:, 1] != 0)
            env.reset(mask=m); ref.reset(m.cpu().numpy().astype(np.uint8))
            counts, rows, ids = env.legal_slab()
    assert env.status() == 0


def test_stepping_calls_are_graph_capturable(pkg):
    """Every launch of the stepping API goes to the caller's current stream and nothing in it synchronises, so a caller
    can capture its loop in a hipGraph (torch.cuda.graph) and replay it: 3 replays of 8 captured iterations (observe +
    select_slab + step_slab, and the fused policy step) == the same 24 iterations issued one by one."""
    T, K = 777, 8
    a = pkg.BatchedEnv(T, seed=8, device=_dev())
    b = pkg.BatchedEnv(T, seed=8, device=_dev())
    a.reset(); b.reset(); a.legal_slab(); b.legal_slab()
    q = torch.rand((T, a.slab_stride), dtype=torch.float32, device=_dev())
    fa = torch.empty((T, 6, 15, 4), dtype=torch.float32, device=_dev())
    fb = torch.empty_like(fa)
    ca = torch.empty(T, dtype=torch.int32, device=_dev())
    cb = torch.empty_like(ca)

    def body(env, face, choice):
        for k in range(K):
            if k % 2:
                env.policy_step_slab(q, 0.25, face_variant=3, face_out=face)
            else:
                env.observe(3, out=face)
                env.select_slab(q, 0.25, out=choice)
                env.step_slab(choice, pkg.STEP_CHOICE, auto_reset=True)

    body(a, fa, ca); body(b, fb, cb)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            body(a, fa, ca)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        g.replay()
        body(b, fb, cb)
    torch.cuda.synchronize()
    assert torch.equal(a.state, b.state) and torch.equal(fa, fb) and torch.equal(a.counts, b.counts)
    assert a.status() == 0 and a.stats() == b.stats()


@pytest.mark.parametrize("T", [1, 5, 9])
def test_slab_api_tiny_table_counts(pkg, oracle, T):
    """fewer tables than a block has waves (T = 1, 5) and one table more than a block (9): the slab loop in every mode
    and the fused policy step against the oracle / the separate launches."""
    rng = np.random.default_rng(T)
    env = pkg.BatchedEnv(T, seed=77, device=_dev())
    fus = pkg.BatchedEnv(T, seed=77, device=_dev())
    ref = oracle.OracleEnv(T, seed=77)
    env.reset(); ref.reset(); fus.reset()
    counts, rows, ids = env.legal_slab()
    fus.legal_slab()
    for it in range(80):
        roff, rrows, rids = ref.legal()
        n = np.diff(roff)
        assert np.array_equal(counts.cpu().numpy(), n)
        take = np.arange(env.slab_stride)[None, :] < n[:, None]
        assert np.array_equal(ids.cpu().numpy()[take], rids) and np.array_equal(rows.cpu().numpy()[take], rrows)
        q = torch.rand((T, env.slab_stride), dtype=torch.float32, device=_dev())
        choice = fus.select_slab(q).cpu().numpy()                # the greedy index over q: what the fused step will play
        mode = it % 3
        if mode == 0:
            sel, gm, om = choice, pkg.STEP_CHOICE, oracle.STEP_CHOICE
        elif mode == 1:
            sel = np.zeros((T, 16), np.int8)
            sel[:] = rrows[roff[:-1] + choice]
            gm, om = pkg.STEP_ROWS, oracle.STEP_ROWS
        else:
            sel = rids[roff[:-1] + choice].astype(np.int32)
            gm, om = pkg.STEP_IDS, oracle.STEP_IDS
        done, r, ill = env.step_slab(torch.from_numpy(sel).to(_dev()), gm, auto_reset=True)
        rdone, rr, rill, _ = ref.step(om, sel, auto_reset=True)
        fd, fr, fi, face = fus.policy_step_slab(q, 0.0, face_variant=int(rng.integers(0, 4)))
        assert np.array_equal(done.cpu().numpy(), rdone) and np.array_equal(r.cpu().numpy(), rr) and not ill.any()
        assert np.array_equal(env.state_export().cpu().numpy(), ref.state), it
        assert torch.equal(fus.state, env.state) and torch.equal(fd, done) and torch.equal(fr, r), it
        assert torch.equal(fus.counts, env.counts)
    assert env.status() == 0 and fus.status() == 0
