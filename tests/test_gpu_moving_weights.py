"""GPU (-m gpu): acting on moving weights -- the seam between the learner and everything that plays from a QNet.

Every front end keeps tables derived from the weights alone (dqn_glue.FactorisedQ / RoleQ) behind a version tuple.  Here a weight
moves (tests/moving_weights_cases.py: an optimizer step, an in-place write, load_state_dict, assign=True, a swapped Parameter, one
tensor alone, a write through .data) under a LIVE object, and the object is asked for Q values:

  eager      the long-lived object's output equals, bit for bit on the valid entries, the output of an object of the same class
             built after the move (same kernels, same summation order: nothing to tolerate); both lie within 1e-5 of the fp64
             literal forward on the current weights (tests/test_gpu_qnet.py's bound, |q| < 1 asserted); the output before the move
             differs from the one after by more than 1e-4 on at least half of the entries, and the REFERENCE moves by more than
             1e-3 in the median (assert_moved: the guard against a vacuous test is on the reference alone).
  captured   a graph holds addresses, and no Python runs at replay.  The contract (dqn_glue._Loop.capture): the derived tables
             have fixed storage written in place; after a learner step the caller runs loop.refresh() and replays -- equal to
             eager steps of a twin; without refresh() the graph plays the weights of the last refresh -- equal to a twin frozen
             on a deep copy -- and never memory that a rebinding refresh handed back to the allocator (blocks of the tables'
             sizes are taken, filled with NaN and dropped before the replay: the test only reads memory that stays mapped).
  .data      a write through p.data is not visible to the version tuple: stale, bit for bit, until refresh(force=True).

T = 192 tables after 12 to 14 random plies (leads, follows and passes in the lists, every role to move); one joker-kicker environment, variant 3 only."""
import copy
import importlib

import pytest
import torch

import moving_weights_cases as M

pytestmark = pytest.mark.gpu

T = 192
PLIES = 12
# face variant -> (gemm, shared) of the PolicyLoop under test: both dense GEMMs and every shared form once each
FORMS = {0: ("torch", False), 1: ("torch", True), 2: ("mfma", False), 3: ("torch", "all")}
CASES = [(0, False), (1, False), (2, False), (3, False), (3, True)]          # (face variant, joker kickers)
Q_REWARD = {"up": 0.5, "lord": 1.0, "down": 0.5}   # (small rewards: an untrained network's leaf values spread over many units)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("doudizhu-rl_amd")


@pytest.fixture(scope="module")
def glue():
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


def _dev():
    return torch.device("cuda:0")


def _net(glue, P, seed):
    torch.manual_seed(seed)
    return glue.QNet(P).to(_dev()).eval()


def _make_env(pkg, seed, jk=False, tables=T):
    """seeded, reset, PLIES random plies; then a third of the tables stays there, a third goes one ply further and a third two:
    lock-step tables would all have the same actor, and the role maps need every role to move in every iteration"""
    env = pkg.BatchedEnv(tables, seed=seed, device=_dev(), native_joker_kickers=jk)
    env.reset()
    for _ in range(PLIES):
        env.step_random()
    rows = env.state_export().view(tables, -1)
    for third in (1, 2):
        env.step_random()
        rows[third::3] = env.state.view(tables, -1)[third::3]
    env.state_import(rows)
    env.legal_slab()
    assert sorted(env.role.unique().tolist()) == [0, 1, 2]
    return env


_positions = {}


def position(pkg, variant, jk):
    """the shared position of the eager tests, made once and only read afterwards: the environment, its face, the valid mask,
    the CSR copy of the lists and a sample of (table, row) pairs for the fp64 reference"""
    key = (variant, jk)
    if key not in _positions:
        env = _positions.get(("env", jk)) or _make_env(pkg, 40 + jk, jk)
        _positions[("env", jk)] = env
        face = env.observe(variant)
        counts = env.counts.long()
        valid = torch.arange(env.slab_stride, device=_dev())[None, :] < counts[:, None]
        off, rows, _ = env.slab_to_csr(rows_per_table=512)
        n = int(off[-1])
        off, rows = off.clone(), rows[:n].clone()
        table = torch.repeat_interleave(torch.arange(T), counts.cpu())
        assert n == int(valid.sum()) == table.numel() and env.status() == 0
        sizes = {"pass only": int((counts == 1).sum()), "short": int(((counts > 1) & (counts <= 15)).sum()), "long": int((counts > 15).sum())}
        assert all(sizes.values()), sizes                                  # forced passes, follows and leads are all in the lists
        pick = torch.arange(0, n, max(1, n // 400))                          # ~400 rows for the fp64 literal network
        _positions[key] = dict(env=env, face=face, valid=valid, off=off, rows=rows, n=n, pick=pick,
                               ref_face=face.cpu()[table[pick]], ref_rows=rows.cpu()[pick])
    return _positions[key]


def _reference(net, pos):
    return M.reference_q(net, pos["ref_face"], pos["ref_rows"])


def _anchored(q_valid, ref, pos, what):
    err = float((q_valid.cpu().double()[pos["pick"]] - ref).abs().max())
    print(f"{what}: max |q - fp64 literal| = {err:.3g}")
    assert err < M.Q_BOUND, (what, err)


def _moved(before, after, what):
    frac = float(((after - before).abs() > 1e-4).float().mean())
    print(f"{what}: {frac:.3f} of the entries moved by more than 1e-4")
    assert frac >= 0.5, (what, frac)


class FrontEnds:
    """every eager front end of one network on one shared position; outputs() -> {name: tensor of the valid entries}"""

    def __init__(self, glue, net, variant, pos):
        env = pos["env"]
        gemm, shared = FORMS[variant]
        self.glue, self.net, self.pos, self.variant = glue, net, pos, variant
        self.policy = glue.PolicyLoop(env, net, face_variant=variant, gemm=gemm, shared=shared)
        self.seat = glue.SeatLoop(env, {"lord": net, "down": net, "up": net}, variant) if variant else None
        self.fq = glue.FactorisedQ(net)

    def refresh(self, force=False):
        done = [self.policy.refresh(force), self.fq.refresh(force), self.net._ddz_factorised.refresh(force)]
        if self.seat is not None:
            done.append(self.seat.refresh(force))
        return done

    def outputs(self):
        pos, env, valid = self.pos, self.pos["env"], self.pos["valid"]
        gemm, shared = FORMS[self.variant]
        out = {"policy": self.policy.q_values()[valid].clone()}
        if self.seat is not None:
            q = self.seat.q_values()
            assert bool((self.seat.slot >= 0).all())
            out["seat"] = q[valid].clone()
        out["ragged"] = self.glue.ragged_q(self.net, pos["face"], pos["rows"], pos["off"]).clone()
        nu = self.fq.needed(env, pos["face"], gemm=gemm, shared=shared)
        rows_in_use = int(nu.seg[15])
        assert 0 < rows_in_use <= nu.d.shape[0]
        out["h0"], out["d"] = nu.h0.clone(), nu.d[:rows_in_use].clone()
        return out


@pytest.mark.parametrize("variant,jk", CASES)
@pytest.mark.parametrize("move", M.MOVES)
def test_eager_front_ends_play_the_moved_weights(pkg, glue, move, variant, jk):
    """PolicyLoop.q_values, SeatLoop.q_values (face variants 1..3), ragged_q and FactorisedQ.needed's h0 / d, each held across
    the move: the sharp check, the anchor, the not-a-no-op check and the reference's own guard of the module docstring.  A write
    through .data: stale bit for bit (the documented behaviour), and a fresh object's output after refresh(force=True)."""
    seen = M.MOVES[move][1]
    pos = position(pkg, variant, jk)
    net = _net(glue, pkg.FACE_PLANES[variant], 50 + variant)
    live = FrontEnds(glue, net, variant, pos)
    before, ref_before = live.outputs(), _reference(net, pos)
    for k in ("policy", "seat", "ragged"):
        if k in before:
            _anchored(before[k], ref_before, pos, f"{k} before {move}")
    M.apply(move, glue, net, seed=6)
    ref = _reference(net, pos)
    print(f"{move}, variant {variant}: fp64 median |dq| = {M.assert_moved(ref_before, ref):.4g}")
    after = live.outputs()
    if not seen:
        for k in before:
            assert torch.equal(after[k], before[k]), (k, "a .data write is not seen: the cached tables are played")
        assert all(live.refresh(force=True))
        after = live.outputs()
    fresh = FrontEnds(glue, net, variant, pos)
    fresh.net._ddz_factorised = glue.FactorisedQ(net)                       # (ragged_q's cached object as well)
    want = fresh.outputs()
    assert sorted(want) == sorted(after)
    for k in want:
        assert torch.equal(after[k], want[k]), (k, "the long-lived object and one built after the move differ")
    for k in ("policy", "seat", "ragged"):
        if k in after:
            _anchored(after[k], ref, pos, f"{k} after {move}")
            _moved(before[k], after[k], f"{k}, {move}")
    assert pos["env"].status() == 0


# ---- RoleQ maps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move,variant", [(m, 3) for m in M.SEEN] + [("adam", 1), ("load", 2)])
def test_role_maps_rewrite_the_moved_slot_and_no_other(pkg, glue, move, variant):
    """Three distinct networks; lord and down sharing one object with up on a second; one role left to the rule agent: ONE
    network moves, the live SeatLoop equals one built after the move (bit for bit on the network tables, the rule tables'
    NaN sentinel untouched), the moved slot's stacked tables changed and every other slot's did not, bit for bit."""
    pos = position(pkg, variant, False)
    env, valid, P = pos["env"], pos["valid"], pkg.FACE_PLANES[variant]
    A, B, C = (_net(glue, P, 60 + s) for s in range(3))
    role = env.role.long()
    for i, (nets, moved) in enumerate((({"lord": A, "down": B, "up": C}, B), ({"lord": A, "down": A, "up": B}, A),
                                       ({"lord": A, "down": A, "up": B}, B), ({"lord": None, "down": B, "up": C}, C))):
        live = glue.SeatLoop(env, nets, variant)
        rq = live.rq
        slot = [s for s, n in enumerate(rq.nets) if n is moved]
        assert len(slot) == 1
        q0 = live.q_values().clone()
        old = {k: getattr(rq, k).clone() for k in rq.STACKED}
        addresses = {k: getattr(rq, k).data_ptr() for k in rq.STACKED}
        M.apply(move, glue, moved, seed=7 + i)
        q1 = live.q_values().clone()
        fresh = glue.SeatLoop(env, nets, variant)
        want = fresh.q_values()
        net_tables = (live.slot >= 0)[:, None] & valid
        assert torch.equal(live.slot, fresh.slot) and torch.equal(q1[net_tables], want[net_tables])
        assert bool(torch.isnan(q1[live.slot < 0]).all())
        of_moved = (torch.tensor(rq.net_of_role, device=_dev())[role] == slot[0])[:, None] & valid
        others = net_tables & ~of_moved
        assert bool(of_moved.any()) and torch.equal(q1[others], q0[others])
        _moved(q0[of_moved], q1[of_moved], f"map {i}, the moved network's tables")
        for k in rq.STACKED:
            now = getattr(rq, k)
            assert now.data_ptr() == addresses[k] and torch.equal(now, getattr(fresh.rq, k)), k
            for s in range(rq.N):
                assert (s == slot[0]) or torch.equal(now[s], old[k][s]), (k, s)
        assert any(not torch.equal(getattr(rq, k)[slot[0]], old[k][slot[0]]) for k in rq.STACKED)
    assert env.status() == 0


# ---- QLeaf ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", M.MOVES)
def test_qleaf_kept_across_a_move_searches_on_the_moved_weights(pkg, glue, move):
    """Eight roots of the shared position, guided search of budget 16 with 2 trees (16 items), one QLeaf kept across two runs
    with a move between them: the leaf values of every step and the final visits / wins of the second run equal those of a QLeaf
    built after the move, exactly.  That the move matters is shown on the fresh objects' own values -- the leaf values of the
    run before and of the run after differ somewhere -- since no fp64 statement of the int32 leaf values exists (the q values
    under them are anchored to the literal network by the eager test above)."""
    seen = M.MOVES[move][1]
    variant, pos = 3, position(pkg, 3, False)
    env = pkg.BatchedEnv(8, seed=41, device=_dev())
    env.state_import(pos["env"].state.view(T, -1)[:8].clone())
    env.legal_slab()
    nets = {r: _net(glue, 6, 70 + k) for k, r in enumerate(glue.ROLE_ORDER)}

    def run(leaf):
        seen_values = []

        def evaluator(search):
            leaf(search)
            seen_values.append(search.values.clone())
        visits, wins = env.guided(16, trees=2, mode="sides", salt=3).run(evaluator)
        return torch.stack(seen_values), visits.clone(), wins.clone()

    kept = glue.QLeaf(nets, variant, reward_dict=Q_REWARD)
    first = run(kept)
    assert kept.refresh() is False
    for net in nets.values():
        M.apply(move, glue, net, seed=8)
    second = run(kept)
    if not seen:
        assert all(torch.equal(a, b) for a, b in zip(first, second))       # stale: the documented behaviour of a .data write
        assert kept.refresh(force=True) is True
        second = run(kept)
    want = run(glue.QLeaf(nets, variant, reward_dict=Q_REWARD))
    for a, b, what in zip(second, want, ("values", "visits", "wins")):
        assert torch.equal(a, b), what
    assert not torch.equal(first[0], want[0]), "the leaf values did not move"
    assert len(set(want[0].flatten().tolist())) > 8 and int(want[1].sum()) > 0
    assert env.status() == 0 and kept.loop.env.status() == 0


# ---- TrainLoop, eager, a learner step after every iteration -----------------------------------------------------------------------
def _td_batch(net, seed, n=32):
    b = M.synthetic_batch(net, seed, n)
    c = M.synthetic_batch(net, seed + 1, n)
    g = torch.Generator().manual_seed(seed)
    return {"s0": b["s0"], "a0": b["a0"], "s1": c["s0"], "a1": c["a0"], "reward": b["ret"],
            "done": (torch.rand(n, generator=g) < 0.3).to(_dev())}


@pytest.mark.parametrize("targets", ["td", "mc"])
def test_train_loop_acts_on_the_weights_of_every_learner_step(pkg, glue, targets):
    """Six iterations of TrainLoop.step() at epsilon 0.1 with one learner step (td_step / mc_step, Adam as train() builds it, a
    synthetic batch) after each.  The twin environment starts from the same state and acts, each iteration, with a SeatLoop
    constructed IN that iteration from the same networks: the ids played, done, r and the whole packed state are equal at every
    iteration (the epsilon draws are the engine's keyed RNG: the twins agree by construction, so any difference is the weights
    the long-lived loop acted on)."""
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    variant = 2
    nets = {"lord": _net(glue, 9, 80), "down": _net(glue, 9, 81), "up": None}
    target = {r: copy.deepcopy(n) for r, n in nets.items() if n is not None}
    opt = {r: torch.optim.Adam(n.parameters(), glue.LEARNING_RATE) for r, n in nets.items() if n is not None}
    a, b = _make_env(pkg, 42), _make_env(pkg, 42)
    assert torch.equal(a.state, b.state)
    loop = glue.TrainLoop(a, nets, variant, capacity=1024, epsilon=0.1, targets=targets)
    eps = {"lord": 0.1, "down": 0.1, "up": 0.0}
    acted = []
    for it in range(6):
        done, r, _ = loop.step()
        ids_a = loop.seat.ids.clone()
        twin = glue.SeatLoop(b, nets, variant, epsilon=eps, auto_reset=False)
        ids_b = twin.act().clone()
        done_b, r_b, illegal_b = b.step_slab(ids_b, engine.STEP_IDS, auto_reset=False)
        assert torch.equal(ids_a, ids_b) and torch.equal(done, done_b) and torch.equal(r, r_b) and not bool(illegal_b.any())
        b.reset(mask=done_b)
        b.legal_slab()
        assert torch.equal(a.state, b.state), it
        acted.append(ids_a)
        role = ("lord", "down")[it % 2]
        if targets == "td":
            glue.td_step(nets[role], target[role], opt[role], _td_batch(nets[role], 90 + it))
        else:
            glue.mc_step(nets[role], opt[role], M.synthetic_batch(nets[role], 90 + it))
    assert a.status() == 0 and b.status() == 0 and a.stats() == b.stats()
    assert len({tuple(x.tolist()) for x in acted}) == 6


# ---- the captured contract --------------------------------------------------------------------------------------------------------
def _tables_of(loop):
    """(name, tensor) of every derived table a graph of the loop holds the address of"""
    if hasattr(loop, "fq"):
        fq = loop.fq
        return [(k, getattr(fq, k)) for k in fq.TABLES] + [("Wd", fq.Wd)]
    rq = loop.seat.rq if hasattr(loop, "seat") else loop.rq
    out = [(k, getattr(rq, k)) for k in rq.STACKED]
    for s, fq in enumerate(rq.fqs):
        out += [(f"{k}[{s}]", getattr(fq, k)) for k in fq.TABLES]
    return out


def _reuse_freed_blocks(shapes):
    """take blocks of the derived tables' sizes from the caching allocator, fill them with NaN and drop them: had a refresh
    rebound a table, its old block would be among these"""
    for _ in range(3):
        held = [torch.full(s, float("nan"), dtype=torch.float32, device=_dev()) for s in shapes]
        torch.cuda.synchronize()
        del held


LOOPS = {
    "policy_dense": lambda glue, env, nets: glue.PolicyLoop(env, nets["lord"], face_variant=3, epsilon=0.1, shared=False),
    "policy_all": lambda glue, env, nets: glue.PolicyLoop(env, nets["lord"], face_variant=3, epsilon=0.1, shared="all"),
    "seat": lambda glue, env, nets: glue.SeatLoop(env, nets, 3, epsilon=0.1),
    "train_td": lambda glue, env, nets: glue.TrainLoop(env, nets, 3, capacity=1024, epsilon=0.1, targets="td"),
    "train_mc": lambda glue, env, nets: glue.TrainLoop(env, nets, 3, capacity=1024, epsilon=0.1, targets="mc"),
}


def _same(la, lb, new_twin=False):
    """states, faces, choices / ids, q and stats of two loops on twin environments, bit for bit.  q: the buffers hold the values of
    the last pass (whose lists the step has replaced since) and, beyond them, of earlier passes: twins with one history are
    compared whole; a twin made just now (new_twin) on the entries it has written since -- everything that left its initial fill,
    0 in a PolicyLoop and NaN in a SeatLoop."""
    torch.cuda.synchronize()
    a, b = la.env, lb.env
    assert torch.equal(a.state, b.state) and torch.equal(a.counts, b.counts) and torch.equal(la.face, lb.face)
    if hasattr(la, "fq"):
        written = (lb.q != 0) if new_twin else torch.ones_like(lb.q, dtype=torch.bool)
        assert torch.equal(la.choice, lb.choice) and bool(written.any()) and torch.equal(la.q[written], lb.q[written])
    else:
        sa, sb = (la.seat, lb.seat) if hasattr(la, "seat") else (la, lb)
        net = sa.slot >= 0                                                  # (choice: valid for the network tables)
        assert torch.equal(sa.ids, sb.ids) and torch.equal(sa.slot, sb.slot) and torch.equal(sa.choice[net], sb.choice[net])
        assert bool(net.any()) and not bool(net.all())                      # the rule agent moves in the same iteration
        written = ~torch.isnan(sb.q)
        assert bool(written.any()) and torch.equal(sa.q[written], sb.q[written])
        assert new_twin or torch.equal(torch.isnan(sa.q), torch.isnan(sb.q))
        if not new_twin and hasattr(la, "rec"):
            for role in ("lord", "down"):
                assert int(la.rec.count(role)) == int(lb.rec.count(role))
                assert torch.equal(la.rec.rings[1 if role == "lord" else 2], lb.rec.rings[1 if role == "lord" else 2])
    assert a.status() == 0 and b.status() == 0 and a.stats() == b.stats()


@pytest.mark.parametrize("kind", LOOPS)
def test_captured_loop_refresh_then_replay_plays_the_moved_weights(pkg, glue, kind):
    """capture(2) after two warm iterations; one replay == two eager steps of a twin loop on a twin environment holding the same
    network objects.  Then, twice (an Adam step, then load_state_dict): a move, loop.refresh(), replay == the twin's two eager
    steps (it refreshes itself), and the storage of every derived table is where the graph recorded it.  Then the other half of
    the contract: a twin frozen on a deep copy of the networks, a move, NO refresh, blocks of the tables' sizes taken from the
    allocator, filled with NaN and dropped, replay == the frozen twin's two eager steps -- the weights of the last refresh,
    not freed memory.  Last: weights that moved while a stream captures raise."""
    nets = {"lord": _net(glue, 6, 101), "down": _net(glue, 6, 102), "up": None}
    a, b = _make_env(pkg, 43), _make_env(pkg, 43)
    la, lb = LOOPS[kind](glue, a, nets), LOOPS[kind](glue, b, nets)
    la.run(2); lb.run(2)                                                      # workspaces allocated, libraries warm
    g = la.capture(2)
    addresses = [(k, t.data_ptr()) for k, t in _tables_of(la)]
    g.replay(); lb.run(2)
    _same(la, lb)
    live = [n for n in nets.values() if n is not None][:1 if kind.startswith("policy") else 2]
    for i, move in enumerate(("adam", "load")):
        for j, net in enumerate(live):
            M.apply(move, glue, net, seed=9 + i + 10 * j)
        assert la.refresh() is True and la.refresh() is False
        assert [(k, t.data_ptr()) for k, t in _tables_of(la)] == addresses
        g.replay(); lb.run(2)
        _same(la, lb)
    # no refresh: the graph plays the weights of the last refresh
    frozen = {r: copy.deepcopy(n) for r, n in nets.items()}
    lf = LOOPS[kind](glue, b, frozen)
    shapes = [tuple(t.shape) for _, t in _tables_of(la)]
    for net in live:
        M.apply("perturb", glue, net, seed=11)
    _reuse_freed_blocks(shapes)
    g.replay(); lf.run(2)
    _same(la, lf, new_twin=True)
    assert la.refresh() is True
    # weights that move while the stream captures: a refresh is never baked into a graph unnoticed
    for net in live:
        M.apply("perturb", glue, net, seed=12)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(graph, stream=side):
                la.face.add_(0.0)                                              # (one node: the graph that is thrown away is not empty)
                la.refresh()
    torch.cuda.current_stream().wait_stream(side)
    assert la.refresh() is True and a.status() == 0
